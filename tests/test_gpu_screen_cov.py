"""gv_screen_cov_set / gv_screen_cov_dev and capi.Shard.screen_cov: the covariate-adjusted association screen on
the two shapes of tests/bed_fixed_restatement.py, with the covariates and phenotypes of tests/screen_cov_restatement.py -- an
ancestry-like, an age-like and a 0 / 1 covariate, a fourth one built on marker TRIP, and the five phenotypes of the marginal screen's
test plus covariate effects.

Bars.  r, t, beta, se: the restatement is evaluated in long double and in plain float64; the GPU (another summation tree) is allowed 16
times the deviation of the float64 form, never less than 1e-12 (the rule of section 15, as tests/test_gpu_screen.py applies it):
|dr| / (|r| + its sampling noise), |dt| / (|t| + 1), |d beta| / (|beta| + se), |d se| / se.  p: against the decimal reference of
tests/student_t_reference.py at the device's own t with nu = n - 2 - K, |p / p_ref - 1| <= 2^-52 (1024 + 16 |ln p|), on at most 64
entries.  The phenotype that is exactly collinear with a marker once the covariates are taken out is decided by the last bits of rho on
every side: it is held to the rule and left out of the deviations.  The set of NaN markers is exact: tests/test_screen_cov_cpu.py asserts
that no variance-inflation factor of these fixtures lies within 1e-9 of a threshold."""
import itertools
import math

import numpy as np
import pytest

import bed_fixed_restatement as bx
import screen_cov_restatement as sc
import screen_restatement as sr
import student_t_reference as st
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
_CACHE = {}
U64 = np.uint64


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def _covs(name, which):
    fx = sc.fixture(name)
    if which == "none":
        return None
    if which.startswith("random"):
        return sc.random_covariates(fx["cs"], int(which[6:]))
    return fx["Cov"][:3] if which == "three" else fx["Cov"]


def _refs(name, which, vif=sc.VIF):
    """the two evaluations of the restatement (long double, float64) for one covariate set: computed once, shared, never changed"""
    key = (name, which, vif)
    if key not in _CACHE:
        fx = sc.fixture(name)
        cs = fx["cs"]
        args = (cs["bed"], cs["N"], cs["M"], cs["present"], fx["Y"], _covs(name, which))
        _CACHE[key] = (sc.screen_cov(*args, vif_max=vif), sc.screen_cov(*args, vif_max=vif, dtype=np.float64))
    return _CACHE[key]


def _shard(cs, kernel="1", m4=None, nonas=None):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GV_ATXM_KERNEL", kernel)
        sh = capi.Shard(cs["N"], cs["M"])
    sh.set_layout(False, 2)
    sh.upload_bed(cs["bed"])
    m4 = cs["m4"] if m4 is None else m4
    if m4 is not None:
        sh.set_mask(m4, cs["nonas"] if nonas is None else nonas)
    sh.compute_markers_statistics()
    return sh


def _envelope(p_ref):
    return 2.0 ** -52 * (1024.0 + 16.0 * abs(math.log(p_ref)))


def _same(a, b):
    return all(np.array_equal(a[k].view(U64), b[k].view(U64)) for k in sc.NAMES)


def _nan_set(got, want):
    for k in sc.NAMES:
        nan = np.isnan(got[k])
        assert np.array_equal(np.nonzero(nan.any(axis=0))[0], sorted(want)), (k, np.nonzero(nan.any(axis=0))[0])
        assert np.all(nan[:, sorted(want)]), k


def _hold(label, got, ref, r64, nu, skip):
    dev64, devg = sc.deviation(r64, ref, nu, skip), sc.deviation(got, ref, nu, skip)
    for k in ("r", "t", "beta", "se"):
        bound = max(16.0 * dev64[k], 1e-12)
        print("%s %s: float64 dev %.3e  GPU dev %.3e  bound %.3e" % (label, k, dev64[k], devg[k], bound))
    for k in ("r", "t", "beta", "se"):
        assert devg[k] <= max(16.0 * dev64[k], 1e-12), (label, k, devg[k], dev64[k])
    keep = np.isfinite(got["t"])
    assert np.all(np.sign(got["t"][keep]) == np.sign(got["r"][keep])) and np.all(np.sign(got["beta"][keep]) == np.sign(got["r"][keep]))
    assert np.all(got["se"][keep] > 0)


@pytest.mark.parametrize("kernel", ["1", "0"], ids=["kernel", "fallback"])
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_five_outputs_against_the_restatement_and_the_decimal_tail(name, kernel):
    fx = sc.fixture(name)
    cs, Y, near, coll = fx["cs"], fx["Y"], fx["near"], fx["coll"]
    ref, r64 = _refs(name, "three")
    n, M, nu = cs["nonas"], cs["M"], cs["nonas"] - 2 - 3
    with _shard(cs, kernel) as sh:
        got = sh.screen_cov(Y, fx["Cov"][:3])
        assert sh.atxm_info()["path"] == ("kernel" if kernel == "1" else "fallback") and sh.atxm_info()["columns"] == 5
        info = sh.screen_cov_info()
        assert info["K"] == 3 and info["nu"] == nu == ref["nu"] and info["columns"] == 5 and info["cached_bytes"] >= 8 * (3 * cs["npad"] + M)
    assert all(got[k].shape == (5, M) for k in sc.NAMES)
    _nan_set(got, [bx.MONO, bx.ALLMISS])
    r, t, p = got["r"], got["t"], got["p"]
    # the exactly collinear entry: the rule, or the last bits of rho short of it
    assert r[4, coll] < -1 + 1e-10 and (t[4, coll] == -np.inf or t[4, coll] < -1e6) and p[4, coll] == 0.0
    assert abs(got["beta"][4, coll] + 2.0) < 1e-6 and 0.0 <= got["se"][4, coll] < 1e-4
    assert r[3, near] > 0.99999 and t[3, near] > 1e3 and abs(got["beta"][3, near] - 1.0) < 1e-3
    _hold("%s %s" % (name, kernel), got, ref, r64, nu, [(4, coll)])
    # p at the device's own t against the decimal reference
    flat = [(c, m) for c in range(5) for m in range(M) if np.isfinite(t[c, m]) and t[c, m] != 0.0]
    fin = sorted(flat, key=lambda cm: abs(t[cm]))
    rows = flat[::max(1, len(flat) // 60)][:62] + [fin[0], fin[-1]]
    assert len(rows) <= 64
    worst = 0.0
    for c, m in rows:
        pr = st.tail(float(t[c, m]), nu)
        if pr is None or float(pr) < 1e-290:
            assert 0.0 <= p[c, m] <= 1e-289, (c, m, t[c, m], p[c, m])
            continue
        pr = float(pr)
        share = abs(p[c, m] / pr - 1.0) / _envelope(pr)
        worst = max(worst, share)
        assert share <= 1.0, (c, m, t[c, m], p[c, m], pr)
    print("%s %s p: worst share of the envelope %.3f over %d entries" % (name, kernel, worst, len(rows)))


def test_the_vif_rule_drops_the_marker_of_the_fourth_covariate_at_50_and_not_at_1e6():
    fx = sc.fixture("ragged")
    cs, Y, coll = fx["cs"], fx["Y"], fx["coll"]
    with _shard(cs) as sh:
        tight = sh.screen_cov(Y, fx["Cov"], vif=sc.VIF)
        loose = sh.screen_cov(Y, False, vif=sc.VIF_LOOSE)              # the covariates of the set before
    ref, r64 = _refs("ragged", "four", sc.VIF_LOOSE)
    assert np.array_equal(np.nonzero(_refs("ragged", "four")[0]["dropped"] & ~ref["novar"])[0], [sc.TRIP]) and not ref["dropped"].any()
    _nan_set(tight, [bx.MONO, bx.ALLMISS, sc.TRIP])
    _nan_set(loose, [bx.MONO, bx.ALLMISS])
    keep = np.setdiff1d(np.arange(cs["M"]), [sc.TRIP])
    assert all(np.array_equal(tight[k][:, keep].view(U64), loose[k][:, keep].view(U64)) for k in sc.NAMES)
    _hold("ragged K = 4", loose, ref, r64, cs["nonas"] - 2 - 4, [(4, coll)])


@pytest.mark.parametrize("which", ["none", "random16", "random17", "random32"])
def test_no_covariate_and_both_widths_of_the_panel_kernels(which):
    fx = sc.fixture("ragged")
    cs, Y, coll = fx["cs"], fx["Y"], fx["coll"]
    Cov = _covs("ragged", which)
    K = 0 if Cov is None else len(Cov)
    ref, r64 = _refs("ragged", which)
    with _shard(cs) as sh:
        got = sh.screen_cov(Y, Cov)
        assert sh.screen_cov_info()["K"] == K and sh.screen_cov_info()["nu"] == cs["nonas"] - 2 - K
    _nan_set(got, [bx.MONO, bx.ALLMISS])
    _hold("ragged %s" % which, got, ref, r64, cs["nonas"] - 2 - K, [(4, coll)])


def test_a_column_is_the_same_bits_alone_among_9_and_among_33_and_twice():
    fx = sc.fixture("ragged")
    cs = fx["cs"]
    N, pres = cs["N"], cs["present"]
    rng = np.random.default_rng(77)
    Y = rng.standard_normal((33, N)) * 10.0 ** rng.integers(-3, 4, size=(33, 1))
    Y[:5] = np.where(pres[None, :], fx["Y"], 0.0)
    Y[6, np.nonzero(pres)[0][11]] = np.nan                           # a NaN inside the mask: that column's outputs only
    Y[:, ~pres] = np.nan
    with _shard(cs) as sh:
        sh.screen_cov_set(fx["Cov"][:3])
        all33 = sh.screen_cov(Y, False)
        again = sh.screen_cov(Y, False)
        first9 = sh.screen_cov(Y[:9], False)
        alone = [sh.screen_cov(Y[j], False) for j in range(33)]
        moved = sh.screen_cov(Y[::-1].copy(), False, cols_per_call=7)
    assert _same(all33, again)
    for k in sc.NAMES:
        assert np.all(np.isnan(all33[k][6])), k
        assert np.array_equal(np.nonzero(np.isnan(all33[k]).all(axis=1))[0], [6]), k
        assert np.array_equal(first9[k].view(U64), all33[k][:9].view(U64)), k
        assert np.array_equal(moved[k][::-1].view(U64), all33[k].view(U64)), k
        for j in range(33):
            assert np.array_equal(alone[j][k][0].view(U64), all33[k][j].view(U64)), (k, j)


def test_the_other_products_do_not_move_by_a_bit():
    fx = sc.fixture("ragged")
    cs = fx["cs"]
    rng = np.random.default_rng(5)
    x = rng.standard_normal(cs["M"])
    z = np.where(np.arange(cs["npad"]) < cs["N"], rng.standard_normal(cs["npad"]), 0.0)
    z[:cs["N"]][~cs["present"]] = 0.0
    Y0 = sr.phenotypes(cs)[0][:3]

    def products(sh):
        xs, zs, oa, ot = sh.vecM(x), sh.vecN(z), sh.vecN(), sh.vecM()
        sh.ax_dev(xs, oa)
        sh.atx_dev(zs, ot)
        pc = sh.pca(2, block=4, tol=1e-6, max_iter=4, strict=False)
        return [oa.download(), ot.download(), pc["evec"], pc["eval"]] + list(sh.screen(Y0))

    with _shard(cs) as sh:
        before = products(sh)
        sh.screen_cov(fx["Y"], fx["Cov"][:3])
        after = products(sh)
        got = sh.screen_cov(fx["Y"], False)                          # ... and gv_pca_dev, which shares the work panels, leaves the cache alone
    for a, b in zip(before, after):
        assert np.array_equal(a.view(U64), b.view(U64))
    with _shard(cs) as sh:
        assert _same(got, sh.screen_cov(fx["Y"], fx["Cov"][:3]))


def test_every_combination_of_optional_outputs():
    fx = sc.fixture("ragged")
    cs, Y = fx["cs"], fx["Y"][:2]
    with _shard(cs) as sh:
        full = sh.screen_cov(Y, fx["Cov"][:3])
        ys = [sh.vecN(sh._padN(y)) for y in Y]
        for mask in itertools.product([False, True], repeat=4):
            outs = [[sh.vecM().fill(7.0) for _ in Y]] + [[sh.vecM().fill(7.0) for _ in Y] if on else None for on in mask]
            sh.screen_cov_dev(ys, *outs)
            for name, vs in zip(sc.NAMES, outs):
                if vs is not None:
                    for j, v in enumerate(vs):
                        assert np.array_equal(v.download().view(U64), full[name][j].view(U64)), (mask, name, j)
                        v.free()
        sh.screen_cov_dev([], [])                                    # C == 0 succeeds and does nothing


def test_refusals_by_their_messages_with_nothing_written():
    fx = sc.fixture("ragged")
    cs, Y = fx["cs"], fx["Y"][:2]
    Cov = np.where(cs["present"][None, :], fx["Cov"], 0.0)
    with _shard(cs) as sh, _shard(cs) as other:
        ys, rs, ts = [sh.vecN(sh._padN(y)) for y in Y], [sh.vecM().fill(7.0) for _ in Y], [sh.vecM().fill(7.0) for _ in Y]
        cv = [sh.vecN(sh._padN(c)) for c in Cov[:3]]
        with pytest.raises(capi.GvError, match="gv_screen_cov_set must be called first"):
            sh.screen_cov_dev(ys, rs)
        assert sh.screen_cov_info()["K"] is None and sh.screen_cov_info()["cached_bytes"] == 0
        for K in (-1, 33):
            with pytest.raises(capi.GvError, match="outside 0 .. GV_PCA_MAX_BLOCK"):
                sh.screen_cov_set(cv, K=K)
        with pytest.raises(capi.GvError, match="array of covariate handles is NULL"):
            sh.screen_cov_set(None, K=1)
        with pytest.raises(capi.GvError, match=r"cov\[1\] is NULL"):
            sh.screen_cov_set([cv[0], None])
        with pytest.raises(capi.GvError, match="cov must be N-space"):
            sh.screen_cov_set([cv[0], rs[0]])
        with pytest.raises(capi.GvError, match="belongs to another context"):
            sh.screen_cov_set([cv[0], other.vecN().fill(1.0)])
        with pytest.raises(capi.GvError, match="Cholesky pivot is not positive.*collinear with each other or with the intercept"):
            sh.screen_cov_set([cv[0], cv[1], cv[0]])
        with pytest.raises(capi.GvError, match="covariate 1 is constant over the phenotyped.*collinear with each other or with the intercept"):
            sh.screen_cov_set([cv[0], sh.vecN(sh._padN(np.full(cs["N"], 3.0)))])
        with pytest.raises(capi.GvError, match="gv_screen_cov_set must be called first"):
            sh.screen_cov_dev(ys, rs)                                # a refused set caches nothing
        sh.screen_cov_set(cv)
        sh.screen_cov_dev(ys, rs, ts)
        good = [v.download() for v in rs + ts]
        with pytest.raises(capi.GvError, match="collinear"):
            sh.screen_cov_set([cv[0], cv[0]])                        # ... and leaves the state cached before it as it was
        assert sh.screen_cov_info()["K"] == 3
        for v in rs + ts:
            v.fill(7.0)
        for bad in (float("nan"), float("inf"), 0.5):
            with pytest.raises(capi.GvError, match="vif_max must be a finite number, at least 1"):
                sh.screen_cov_dev(ys, rs, vif=bad)
        with pytest.raises(capi.GvError, match="number of columns is negative"):
            sh._ck(sh.L.gv_screen_cov_dev(sh.h, -1, sh._handles(ys), 50.0, sh._handles(rs), None, None, None, None))
        with pytest.raises(capi.GvError, match="arrays of column handles are NULL"):
            sh.screen_cov_dev(None, rs)
        with pytest.raises(capi.GvError, match="handle of column 1 is NULL"):
            sh.screen_cov_dev(ys, [rs[0], None])
        with pytest.raises(capi.GvError, match="handle of column 0 is NULL"):
            sh.screen_cov_dev(ys, rs, None, None, [None, ts[0]])
        with pytest.raises(capi.GvError, match="y must be N-space, out M-space"):
            sh.screen_cov_dev([rs[0]], [rs[1]])
        with pytest.raises(capi.GvError, match="se must be M-space"):
            sh.screen_cov_dev(ys, rs, None, None, None, [ts[0], ys[1]])     # an input among the outputs
        with pytest.raises(capi.GvError, match="two outputs are the same vector"):
            sh.screen_cov_dev(ys, rs, ts, None, [ts[1], ts[0]])
        with pytest.raises(capi.GvError, match="two outputs are the same vector"):
            sh.screen_cov_dev(ys, rs, None, [rs[1], ts[0]])
        with pytest.raises(capi.GvError, match="belongs to another context"):
            sh.screen_cov_dev(ys, rs, [ts[0], other.vecM()])
        assert all(np.all(v.download() == 7.0) for v in rs + ts)     # nothing was written by a refused call
        sh.screen_cov_dev(ys, rs, ts)
        assert all(np.array_equal(v.download().view(U64), g.view(U64)) for v, g in zip(rs + ts, good))
        # the state gv_screen_dev asks for
        sh.compute_markers_statistics(0.5)
        with pytest.raises(capi.GvError, match="alpha_scale = 1"):
            sh.screen_cov_set(cv)
        sh.set_mask(cs["m4"], cs["nonas"])
        with pytest.raises(capi.GvError, match="marker statistics must be set first"):
            sh.screen_cov_set(cv)
        with pytest.raises(capi.GvError, match="marker statistics must be set first"):
            sh.screen_cov_dev(ys, rs)
    for what in ("meth", "dosage8"):
        with capi.Shard(64, 32) as sh:
            if what == "meth":
                sh.synth_meth(3)
            else:
                sh.synth_dosage(3, 8)
            with pytest.raises(capi.GvError, match="methylation or dosage"):
                sh.screen_cov_set([sh.vecN().fill(0.0)])
            with pytest.raises(capi.GvError, match="methylation or dosage"):
                sh.screen_cov_dev([sh.vecN().fill(0.0)], [sh.vecM()])
    with capi.Shard(8, 64) as sh:
        sh.set_layout(False, 2)
        sh.synth_bed(3)
        sh.set_mask(np.array([0x03, 0x00], dtype=np.uint8), 2)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="fewer than 3"):
            sh.screen_cov_set(None)
        sh.set_mask(np.array([0x0F, 0x00], dtype=np.uint8), 4)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match=r"leave nu = n - 2 - K = 0 degrees of freedom"):
            sh.screen_cov_set(np.random.default_rng(1).standard_normal((2, 8)))
        sh.screen_cov_set(np.random.default_rng(1).standard_normal((1, 8)))
        assert sh.screen_cov_info()["nu"] == 1
