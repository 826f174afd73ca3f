"""The association screens on dosage data (gv_set_screen_dosage): gv_screen_dev and gv_screen_cov_set /
gv_screen_cov_dev on 8- and 16-bit codes, with and without reserved codes, on either route of the 8-bit products, held to
tests/dosage_screen_restatement.py on its fixtures (515 x 300, a phenotype mask; with missing entries: 5 % reserved codes and three
hand-placed rows -- all missing, one present entry, constant).

Bars.
  r, route 0 and 16-bit codes (fp64 kernels): the restatement in long double and in float64; the GPU is allowed 16 times the deviation of
      the float64 form, never less than 1e-12 (the rule of section 15), in the measure |dr| / (|r| + sqrt((1 - r^2) / nu)).
  r of the marginal screen, route 1: the contract of the fixed-point product in gvamp.h, |dz_m| <= fx.atx_bound(N, scale, msig, u)[m], times
      a = sqrt(N) / (n - 1): derived, not measured.  The adjusted screen on route 1 has two sources of error, and its bar is their sum:
      the fp64 panel arithmetic (the rule of section 15, as on route 0) and the contract of the products, which enters rho = z afac / sqrt(v)
      through z (b / sqrt(v), b = atx_bound at max |u| <= 1 times afac = sqrt(N / (n - 1)): the columns have unit norm) and through
      v = 1 - c sum_k z_k^2 (|d rho| = |rho| |dv| / (2 v) <= sqrt(K) b / v by Cauchy-Schwarz with c sum z_k^2 <= 1): together at most
      (b / sqrt(v)) (1 + sqrt(K) / sqrt(v)).
  t, beta, se: restated in long double from the DEVICE'S OWN r (and the restatement's S, sxx, v), under the rule of section 15 with the
      float64 evaluation of the same expression as the yardstick: |dt| / (|t| + 1), |d beta| / (|beta| + se), |d se| / se.
  p: against the decimal reference of tests/student_t_reference.py at the device's own t, |p / p_ref - 1| <= 2^-52 (1024 + 16 |ln p|), on
      at most 64 entries (the envelope of tests/test_gpu_screen_cov.py).
The entry that is exactly collinear with a marker is decided by the last bits of r on every side: it is held to the rule and left out.
The NaN set is exact: {q == 0} and, adjusted, {VIF > vif_max}; tests/test_dosage_screen_cpu.py asserts that no variance-inflation factor of
these fixtures lies within 1e-9 of a threshold."""
import math

import numpy as np
import pytest

import dosage_fixed_restatement as fx
import dosage_screen_restatement as ds
import student_t_reference as st
import test_gpu_dosage as gd
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
LD = np.longdouble
U64 = np.uint64
NAMES = ds.NAMES
# (bits, reserved codes, requested route): route 1 is in force for 8-bit codes without a reserved code only
CONFIGS = {"u8-route0": (8, False, 0), "u8-route1": (8, False, 1), "u16": (16, False, 0), "u8-na": (8, True, 1), "u16-na": (16, True, 0)}
_CACHE = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL", "GV_ATXM_TILES", "GV_DOSAGE_MFMA_SEG", "GV_DOSAGE_NA_KERNELS"):
        monkeypatch.delenv(k, raising=False)


def _shard(f, route=0, option=1, stats=True):
    sh = capi.Shard(f["N"], f["M"])
    try:
        sh.set_dosage_route(route)
        sh.upload_dosage(f["B"], f["scale"], missing=f["missing"])
        sh.set_mask(f["m4"], f["nonas"])
        if stats:
            sh.compute_markers_statistics()
        sh.set_screen_dosage(option)
    except BaseException:
        sh.close()
        raise
    return sh


def _refs(cfg, which, vif=ds.VIF):
    """the two evaluations of the restatement (long double, float64) of a configuration and covariate set: computed once, shared"""
    bits, missing, _ = CONFIGS[cfg]
    key = (bits, missing, which, vif)
    if key not in _CACHE:
        f = ds.fixture(bits, missing)
        Cov = None if which == "marginal" else _covs(f, which)
        args = (f["B"], bits, f["scale"], missing, f["present"], f["Y0" if which == "marginal" else "Y"], Cov)
        _CACHE[key] = (ds.screen_cov(*args, vif_max=vif), ds.screen_cov(*args, vif_max=vif, dtype=np.float64))
    return _CACHE[key]


def _covs(f, which):
    if which == "none":
        return None
    if which.startswith("random"):
        return ds.random_covariates(f, int(which[6:]))
    return f["Cov"][:3] if which == "three" else f["Cov"]


def _envelope(p_ref):
    return 2.0 ** -52 * (1024.0 + 16.0 * abs(math.log(p_ref)))


def _nan_set(got, want, names):
    for k in names:
        nan = np.isnan(got[k])
        assert np.array_equal(np.nonzero(nan.any(axis=0))[0], sorted(want)), (k, np.nonzero(nan.any(axis=0))[0])
        assert np.all(nan[:, sorted(want)]), k


def _dev_r(r, ref_r, nu, ok):
    with np.errstate(invalid="ignore"):
        noise = np.sqrt(np.maximum(LD(1) - ref_r * ref_r, LD(0)) / LD(nu))
        d = np.abs(np.asarray(r, dtype=LD) - ref_r) / (np.abs(ref_r) + noise)
    return float(np.max(d[ok]))


def _hold_r_rule15(label, got_r, ref, r64, nu, ok, contract=None):
    """contract: per marker, what the fixed-point products may add in absolute terms (route 1 in force); None on the fp64 kernels"""
    dev64 = _dev_r(r64["r"], ref["r"], nu, ok)
    rule = max(16.0 * dev64, 1e-12)
    with np.errstate(invalid="ignore"):
        noise = np.sqrt(np.maximum(LD(1) - ref["r"] * ref["r"], LD(0)) / LD(nu))
        allowed = rule * (np.abs(ref["r"]) + noise) + (0.0 if contract is None else np.asarray(contract, dtype=LD)[None, :])
        ratio = float(np.max((np.abs(np.asarray(got_r, dtype=LD) - ref["r"]) / allowed)[ok]))
    print("%s r: float64 dev %.3e  rule %.3e  largest contract term %.3e  worst |dr| / allowed = %.3e"
          % (label, dev64, rule, 0.0 if contract is None else float(np.max(contract)), ratio))
    assert ratio <= 1.0, (label, ratio, dev64)


def _contract(f, msig, ref, K):
    """the adjusted screen on route 1: (b / sqrt(v)) (1 + sqrt(K) / sqrt(v)) per marker (the module docstring)"""
    n = f["nonas"]
    b = fx.atx_bound(f["N"], f["scale"], msig, np.ones(f["N"])) * math.sqrt(f["N"] / (n - 1.0))
    v = np.where(ref["novar"] | ref["dropped"], 1.0, (1.0 / ref["vif"]).astype(np.float64))
    return b / np.sqrt(v) * (1.0 + math.sqrt(K) / np.sqrt(v))


def _hold_from_r(label, got, ref, nu, ok, adjusted):
    """t (and beta, se) restated from the device's own r in long double, the float64 evaluation of the same expression as the yardstick"""
    r = got["r"]
    t_ld = ds.from_r(r, nu)
    with np.errstate(invalid="ignore", divide="ignore"):
        om64 = 1.0 - r * r
        t_64 = np.where(om64 <= 0, np.copysign(np.inf, r), r * np.sqrt(nu / np.where(om64 <= 0, 1.0, om64)))
    fin = ok & np.isfinite(t_ld)
    meas = {"t": (got["t"], t_64, t_ld, np.abs(t_ld) + 1)}
    if adjusted:
        sxx = np.where(ref["novar"], LD(1), ref["sxx"])
        v = np.where(ref["novar"] | ref["dropped"], LD(1), LD(1) / ref["vif"])
        b_ld, s_ld = ds.beta_se_from_r(r, nu, ref["S"], sxx, v)
        with np.errstate(invalid="ignore", divide="ignore"):
            d64 = (sxx * v).astype(np.float64)[None, :]
            S64 = ref["S"].astype(np.float64)[:, None]
            b_64 = r * np.sqrt(S64 / d64)
            s_64 = np.where(om64 <= 0, 0.0, np.sqrt(S64 * np.where(om64 <= 0, 1.0, om64) / (nu * d64)))
        fin = fin & (s_ld > 0)
        meas["beta"] = (got["beta"], b_64, b_ld, np.abs(b_ld) + s_ld)
        meas["se"] = (got["se"], s_64, s_ld, s_ld)
    for k, (g, f64, ld, scale) in meas.items():
        with np.errstate(invalid="ignore", divide="ignore"):
            devg = float(np.max((np.abs(np.asarray(g, dtype=LD) - ld) / scale)[fin]))
            dev64 = float(np.max((np.abs(np.asarray(f64, dtype=LD) - ld) / scale)[fin]))
        bound = max(16.0 * dev64, 1e-12)
        print("%s %s from the device's r: float64 dev %.3e  GPU dev %.3e  bound %.3e  ratio %.3e" % (label, k, dev64, devg, bound, devg / bound))
        assert devg <= bound, (label, k, devg, dev64)


def _hold_p(label, t, p, nu):
    C, M = t.shape
    flat = [(c, m) for c in range(C) for m in range(M) if np.isfinite(t[c, m]) and t[c, m] != 0.0]
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
        assert share <= 1.0, (label, c, m, t[c, m], p[c, m], pr)
    print("%s p: worst share of the envelope %.3f over %d entries" % (label, worst, len(rows)))


def _ok(ref):
    ok = np.isfinite(ref["r"]) & np.isfinite(ref["t"])
    ok[4, ds.COLL] = False
    return ok


def _collinear_entry(got, adjusted):
    r, t, p = got["r"], got["t"], got["p"]
    assert r[4, ds.COLL] < -1 + 1e-10 and (t[4, ds.COLL] == -np.inf or t[4, ds.COLL] < -1e6) and p[4, ds.COLL] == 0.0
    assert r[3, ds.NEAR] > 0.99999 and t[3, ds.NEAR] > 1e3
    if adjusted:
        assert abs(got["beta"][4, ds.COLL] + 2.0) < 1e-6 and 0.0 <= got["se"][4, ds.COLL] < 1e-4
        assert abs(got["beta"][3, ds.NEAR] - 1.0) < 1e-3


def _route1_r_bound(f, msig, U, n):
    """per column and marker: the contract of the fixed-point ATx at p = u, times a = sqrt(N) / (n - 1)"""
    N = f["N"]
    return np.stack([fx.atx_bound(N, f["scale"], msig, u[:N]) for u in U]) * math.sqrt(N) / (n - 1)


def test_with_the_option_off_both_screens_refuse_with_the_old_words():
    f = ds.fixture(8, False)
    with _shard(f, option=0) as sh:
        assert sh.get_screen_dosage() == 0
        with pytest.raises(capi.GvError, match="gv_screen_dev: no screen is defined for methylation or dosage data"):
            sh.screen(f["Y"][:1])
        with pytest.raises(capi.GvError, match="gv_screen_cov_set: no screen is defined for methylation or dosage data"):
            sh.screen_cov_set(None)
        with pytest.raises(capi.GvError, match="gv_screen_cov_dev: no screen is defined for methylation or dosage data"):
            sh.screen_cov_dev([sh.vecN().fill(0.0)], [sh.vecM()])
        with pytest.raises(capi.GvError, match="on must be 0 or 1"):
            sh.set_screen_dosage(2)
        sh.set_screen_dosage(1)
        assert sh.get_screen_dosage() == 1
        sh.screen(f["Y"][:1])
        sh.set_screen_dosage(0)
        with pytest.raises(capi.GvError, match="methylation or dosage"):
            sh.screen(f["Y"][:1])
    # methylation data stay refused, and the option outlives the dataset
    with capi.Shard(64, 32) as sh:
        sh.set_screen_dosage(1)
        sh.synth_meth(3)
        sh.set_mask(gd.na_mask(64, False)[0], 64)
        sh.compute_markers_statistics()
        assert sh.get_screen_dosage() == 1
        with pytest.raises(capi.GvError, match="methylation or dosage"):
            sh.screen_dev([sh.vecN().fill(0.0)], [sh.vecM()])
        with pytest.raises(capi.GvError, match="methylation or dosage"):
            sh.screen_cov_set(None)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_marginal_screen(cfg):
    bits, missing, route = CONFIGS[cfg]
    f = ds.fixture(bits, missing)
    ref, r64 = _refs(cfg, "marginal")
    n, nu = f["nonas"], f["nonas"] - 2
    with _shard(f, route) as sh:
        in_force = sh.dosage_route()[1]
        assert in_force == (1 if cfg == "u8-route1" else 0)
        r, t, p = sh.screen(f["Y0"])
        info = sh.atxm_info()
        assert info["columns"] == 5 and info["path"] == ("kernel" if in_force else "fallback"), info
        _, msig = sh.marker_stats()
        U = sh.screen_prepare(f["Y0"])
    got = dict(r=r, t=t, p=p)
    assert np.array_equal(np.nonzero(ref["novar"])[0], f["novar"])
    _nan_set(got, f["novar"], ("r", "t", "p"))
    _collinear_entry(got, False)
    ok = _ok(ref)
    if in_force:
        bound = _route1_r_bound(f, msig, U, n)
        err = np.abs(np.asarray(r, dtype=LD) - ref["r"])
        ratio = float(np.max((err / bound)[ok]))
        print("%s r: worst |dr| / (atx_bound sqrt(N) / (n - 1)) = %.3e (largest bound %.3e)" % (cfg, ratio, float(np.max(bound[ok]))))
        assert ratio <= 1.0, (cfg, ratio)
    else:
        _hold_r_rule15(cfg, r, ref, r64, nu, ok)
    _hold_from_r(cfg, got, ref, nu, ok, False)
    keep = np.isfinite(t)
    assert np.all(np.sign(t[keep]) == np.sign(r[keep]))
    _hold_p(cfg, t, p, nu)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_adjusted_screen_with_three_covariates(cfg):
    bits, missing, route = CONFIGS[cfg]
    f = ds.fixture(bits, missing)
    ref, r64 = _refs(cfg, "three")
    n, nu = f["nonas"], f["nonas"] - 2 - 3
    with _shard(f, route) as sh:
        in_force = sh.dosage_route()[1]
        got = sh.screen_cov(f["Y"], f["Cov"][:3])
        info = sh.atxm_info()
        assert info["columns"] == 5 and info["path"] == ("kernel" if in_force else "fallback"), info
        ci = sh.screen_cov_info()
        assert ci["K"] == 3 and ci["nu"] == nu == ref["nu"] and ci["columns"] == 5
        _, msig = sh.marker_stats()
    _nan_set(got, f["novar"], NAMES)
    _collinear_entry(got, True)
    ok = _ok(ref)
    _hold_r_rule15(cfg, got["r"], ref, r64, nu, ok, _contract(f, msig, ref, 3) if in_force else None)
    _hold_from_r(cfg, got, ref, nu, ok, True)
    keep = np.isfinite(got["t"])
    assert np.all(np.sign(got["t"][keep]) == np.sign(got["r"][keep])) and np.all(np.sign(got["beta"][keep]) == np.sign(got["r"][keep]))
    assert np.all(got["se"][keep] > 0)
    _hold_p(cfg, got["t"], got["p"], nu)


@pytest.mark.parametrize("cfg", ["u8-route1", "u8-na", "u16-na"])
def test_the_nan_set_is_q_zero_and_the_vif_rule(cfg):
    """a covariate built on marker TRIP: dropped at vif_max = 50, kept at 1e6; everything else is the same bits"""
    bits, missing, route = CONFIGS[cfg]
    f = ds.fixture(bits, missing)
    with _shard(f, route) as sh:
        tight = sh.screen_cov(f["Y"], f["Cov"], vif=ds.VIF)
        loose = sh.screen_cov(f["Y"], False, vif=ds.VIF_LOOSE)
        in_force, msig = sh.dosage_route()[1], sh.marker_stats()[1]
    ref, r64 = _refs(cfg, "four", ds.VIF_LOOSE)
    assert np.array_equal(np.nonzero(_refs(cfg, "four")[0]["dropped"] & ~ref["novar"])[0], [ds.TRIP]) and not ref["dropped"].any()
    _nan_set(tight, f["novar"] + [ds.TRIP], NAMES)
    _nan_set(loose, f["novar"], NAMES)
    keep = np.setdiff1d(np.arange(f["M"]), [ds.TRIP])
    assert all(np.array_equal(tight[k][:, keep].view(U64), loose[k][:, keep].view(U64)) for k in NAMES)
    _hold_r_rule15(cfg + " K = 4", loose["r"], ref, r64, f["nonas"] - 6, _ok(ref), _contract(f, msig, ref, 4) if in_force else None)


@pytest.mark.parametrize("which", ["none", "random17"])
@pytest.mark.parametrize("cfg", ["u8-route1", "u16-na"])
def test_covariate_counts_0_and_17(cfg, which):
    bits, missing, route = CONFIGS[cfg]
    f = ds.fixture(bits, missing)
    Cov = _covs(f, which)
    K = 0 if Cov is None else len(Cov)
    ref, r64 = _refs(cfg, which)
    nu = f["nonas"] - 2 - K
    with _shard(f, route) as sh:
        got = sh.screen_cov(f["Y"], Cov)
        assert sh.screen_cov_info()["K"] == K and sh.screen_cov_info()["nu"] == nu
        in_force, msig = sh.dosage_route()[1], sh.marker_stats()[1]
        if K == 0:
            marg = sh.screen(f["Y"])
    _nan_set(got, f["novar"], NAMES)
    _hold_r_rule15("%s K = %d" % (cfg, K), got["r"], ref, r64, nu, _ok(ref), _contract(f, msig, ref, K) if in_force else None)
    _hold_from_r("%s K = %d" % (cfg, K), got, ref, nu, _ok(ref), True)
    if K == 0:      # without covariates rho is the marginal r up to the roundings of the two preparations
        fin = _ok(ref)
        assert np.all(np.abs(got["r"][fin] - marg[0][fin]) <= 1e-12)


@pytest.mark.parametrize("route", [0, 1])
def test_a_bed_file_written_as_codes_gives_the_bed_screens(route):
    """hard calls without missing genotypes as codes 64 {0, 1, 2} at scale 2^-6: r, t, p, beta, se of the bed screens to 1e-9 (the bar
    tests/test_gpu_dosage.py holds x_hat of the two kinds to)"""
    N, M = 515, 300
    bed = synth.synth_bed(N, M, seed=21, miss_ppm=0)
    G = gd.decode_bed(bed, N, M)
    m4, pres, nonas = ds.present_mask(N)
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((5, N)) * np.array([[1.0], [1e-3], [50.0], [1.0], [1.0]])
    Y[3] += 0.3 * G[5]
    Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N), (rng.random(N) < 0.5).astype(float)])
    with capi.Shard(N, M) as sb:
        sb.set_layout(False, 2)
        sb.upload_bed(bed)
        sb.set_mask(m4, nonas)
        sb.compute_markers_statistics()
        bm, bc = sb.screen(Y), sb.screen_cov(Y, Cov)
    with capi.Shard(N, M) as sd:
        sd.set_dosage_route(route)
        sd.upload_dosage(gd.bed_as_codes(G, 8), gd.DYADIC[8])
        sd.set_mask(m4, nonas)
        sd.compute_markers_statistics()
        sd.set_screen_dosage(1)
        assert sd.dosage_route() == (route, route)
        dm, dcv = sd.screen(Y), sd.screen_cov(Y, Cov)
    for k, name in enumerate("rtp"):
        assert np.array_equal(np.isnan(dm[k]), np.isnan(bm[k])), name
        fin = np.isfinite(bm[k])
        print("marginal %s rel %.3e" % (name, gd.rel(dm[k][fin], bm[k][fin])))
        assert gd.rel(dm[k][fin], bm[k][fin]) < 1e-9, name
    for name in NAMES:
        assert np.array_equal(np.isnan(dcv[name]), np.isnan(bc[name])), name
        fin = np.isfinite(bc[name])
        print("adjusted %s rel %.3e" % (name, gd.rel(dcv[name][fin], bc[name][fin])))
        assert gd.rel(dcv[name][fin], bc[name][fin]) < 1e-9, name
    assert np.isfinite(bm[0]).sum() > 0.9 * bm[0].size


@pytest.mark.parametrize("cfg", ["u8-route0", "u8-route1", "u16-na"])
def test_a_column_is_the_same_bits_alone_and_among_nine(cfg):
    bits, missing, route = CONFIGS[cfg]
    f = ds.fixture(bits, missing)
    rng = np.random.default_rng(77)
    Y = rng.standard_normal((9, f["N"])) * 10.0 ** rng.integers(-3, 4, size=(9, 1))
    Y[:5] = np.where(f["present"][None, :], f["Y"], 0.0)
    Y[:, ~f["present"]] = np.nan
    with _shard(f, route) as sh:
        all9 = sh.screen(Y)
        assert sh.atxm_info()["path"] == ("kernel" if cfg == "u8-route1" else "fallback")
        alone = [sh.screen(Y[j]) for j in range(9)]
        sh.screen_cov_set(f["Cov"][:3])
        adj9 = sh.screen_cov(Y, False)
        adj_alone = [sh.screen_cov(Y[j], False) for j in range(9)]
        again = sh.screen_cov(Y, False)
    for j in range(9):
        for k in range(3):
            assert np.array_equal(alone[j][k][0].view(U64), all9[k][j].view(U64)), (k, j)
        for name in NAMES:
            assert np.array_equal(adj_alone[j][name][0].view(U64), adj9[name][j].view(U64)), (name, j)
    assert all(np.array_equal(adj9[name].view(U64), again[name].view(U64)) for name in NAMES)


@pytest.mark.parametrize("bits", [8, 16])
def test_device_generated_codes_with_missing_entries(bits):
    """gv_synth_dosage_na, reproduced on the host: the marginal screen against the restatement under the rule of section 15"""
    N, M = 257, 200
    m4, pres, nonas = ds.present_mask(N)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((3, N))
    B = synth.synth_dosage_na(N, M, 3, bits, 50000)
    scale = 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0
    with capi.Shard(N, M) as sh:
        sh.synth_dosage_na(3, bits, 50000)
        sh.set_mask(m4, nonas)
        sh.compute_markers_statistics()
        sh.set_screen_dosage(1)
        assert sh.dosage_info()["reserved"] > 0
        r, t, p = sh.screen(Y)
    ref = ds.screen(B, bits, scale, True, pres, Y)
    r64 = ds.screen(B, bits, scale, True, pres, Y, dtype=np.float64)
    assert np.array_equal(np.isnan(r).any(axis=0), ref["novar"])
    ok = np.isfinite(ref["r"])
    _hold_r_rule15("synth_dosage_na %d bits" % bits, r, ref, r64, nonas - 2, ok)
    _hold_from_r("synth_dosage_na %d bits" % bits, dict(r=r, t=t, p=p), ref, nonas - 2, ok, False)


def test_refusals_by_their_messages():
    f = ds.fixture(8, False)
    Y = f["Y"][:2]
    with _shard(f, 1) as sh, _shard(f, 1) as other:
        us = [sh.vecN(u) for u in sh.screen_prepare(Y)]
        rs, ts = [sh.vecM().fill(7.0) for _ in Y], [sh.vecM().fill(7.0) for _ in Y]
        with pytest.raises(capi.GvError, match="number of columns is negative"):
            sh._ck(sh.L.gv_screen_dev(sh.h, -1, sh._handles(us), sh._handles(rs), None, None))
        with pytest.raises(capi.GvError, match="arrays of column handles are NULL"):
            sh.screen_dev(None, rs)
        with pytest.raises(capi.GvError, match="handle of column 1 is NULL"):
            sh.screen_dev(us, [rs[0], None])
        with pytest.raises(capi.GvError, match="u must be N-space, out M-space"):
            sh.screen_dev([rs[0]], [rs[1]])
        with pytest.raises(capi.GvError, match="two outputs are the same vector"):
            sh.screen_dev(us, rs, [ts[0], rs[0]])
        with pytest.raises(capi.GvError, match="belongs to another context"):
            sh.screen_dev(us, rs, [ts[0], other.vecM()])
        with pytest.raises(capi.GvError, match="gv_screen_cov_set must be called first"):
            sh.screen_cov_dev(us, rs)
        with pytest.raises(capi.GvError, match="outside 0 .. GV_PCA_MAX_BLOCK"):
            sh.screen_cov_set([us[0]], K=33)
        with pytest.raises(capi.GvError, match="covariate 0 is constant over the phenotyped"):
            sh.screen_cov_set(np.full((1, f["N"]), 3.0))
        sh.screen_cov_set(None)
        with pytest.raises(capi.GvError, match="vif_max must be a finite number, at least 1"):
            sh.screen_cov_dev(us, rs, vif=0.5)
        assert all(np.all(v.download() == 7.0) for v in rs + ts)         # nothing was written by a refused call
        sh.screen_dev(us, rs, ts)
        assert all(np.all(v.download()[np.setdiff1d(np.arange(f["M"]), f["novar"])] != 7.0) for v in rs)
        sh.compute_markers_statistics(0.5)
        with pytest.raises(capi.GvError, match="gv_screen_dev: the marker statistics must be those of alpha_scale = 1"):
            sh.screen_dev(us, rs)
        with pytest.raises(capi.GvError, match="gv_screen_cov_set: the marker statistics must be those of alpha_scale = 1"):
            sh.screen_cov_set(None)
    for bits in (8, 16):
        with capi.Shard(8, 64) as sh:
            sh.set_screen_dosage(1)
            sh.synth_dosage(3, bits)
            sh.set_mask(np.array([0x03, 0x00], dtype=np.uint8), 2)
            sh.compute_markers_statistics()
            with pytest.raises(capi.GvError, match="fewer than 3"):
                sh.screen_dev([sh.vecN().fill(0.0)], [sh.vecM()])
            with pytest.raises(capi.GvError, match="fewer than 3"):
                sh.screen_cov_set(None)
            sh.set_mask(np.array([0x0F, 0x00], dtype=np.uint8), 4)
            sh.compute_markers_statistics()
            with pytest.raises(capi.GvError, match=r"leave nu = n - 2 - K = 0 degrees of freedom"):
                sh.screen_cov_set(np.random.default_rng(1).standard_normal((2, 8)))
            sh.screen_cov_set(np.random.default_rng(1).standard_normal((1, 8)))
            assert sh.screen_cov_info()["nu"] == 1
