"""gv_pca_dev / gv_pca_loadings_dev / capi.Shard.pca: principal components of the resident genotypes by block subspace iteration
(DESIGN.md section 24), held to tests/pca_restatement.py: the dense relationship matrix G of the definition and numpy.linalg.eigh of it.

tol = 1e-9, max_iter = 100, the default engine (tile layout, kernel mode 1) unless stated.  eps = 2^-52, lam the eigh spectrum of G,
delta_i = min_{j != i} |theta_i - lam_j|.  pr.check_pairs asserts, in this order:
  1. ||G u_i - theta_i u_i|| <= 1.01 tol theta_i with the restatement's G, and resid[i] within 1 % of that norm (only where that norm is
     itself rounding noise, below 100 N eps lam_1 -- the 5 x 3 shape, whose block spans the range of G -- within N eps lam_1 instead);
  2. sin angle(u_i, e_i) <= r_i / delta_i + N eps (Davis-Kahan), the sine as ||u_i - e_i (e_i^T u_i)||, and
     |theta_i - lam_i| <= r_i^2 / delta_i + N eps lam_1 (Kato-Temple);
  3. max |U^T U - I| <= N eps, NA slots exactly 0, the sign rule, theta descending.
The tests add: pad slots exactly 0, iterations <= the restatement's + 2, converged = 1; bit reproducibility across the products' pins
and a forced multi-rank context; the other engines; the loadings; the context as found; the refusals."""
import numpy as np
import pytest

import pca_restatement as pr
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
TOL, MAX_ITER = 1e-9, 100
PIN_VARS = ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL", "GV_SCORE_COLS", "GV_SCORE_KS", "GV_SCORE_KERNEL")
PINS = {"atxm-cols4": dict(GV_ATXM_COLS="4"), "score-cols4": dict(GV_SCORE_COLS="4"), "score-cols16": dict(GV_SCORE_COLS="16"),
        "atxm-ks3": dict(GV_ATXM_KS="3"), "score-ks3": dict(GV_SCORE_KS="3"), "no-kernels": dict(GV_ATXM_KERNEL="0", GV_SCORE_KERNEL="0"),
        "forced-multi": dict()}
ENGINES = {"two-stripe-sets": dict(layout=1, mode=1), "mode2": dict(layout=2, mode=2), "mode0-raw": dict(layout="raw", mode=0)}
_RUNS = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in PIN_VARS:
        monkeypatch.delenv(k, raising=False)


def _shard(cs, layout=2, mode=1, env=None, stats=True):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        sh = capi.Shard(cs["N"], cs["M"])
    if layout == "raw":
        sh.set_layout(True, 1)
    else:
        sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(cs["bed"])
    sh.set_mask(cs["m4"], cs["nonas"])
    if stats:
        sh.compute_markers_statistics()
    return sh


def _q0(sh, cs, block=None):
    Q = np.zeros((cs["L"], 4 * sh.mbytes))
    Q[:, :cs["N"]] = cs["q0"] if block is None else block
    return Q


def _run(sh, cs, tol=TOL, max_iter=MAX_ITER, block=None, loadings=False):
    """one gv_pca_dev on the case's starting block: dict eval, resid, U (k x 4 mbytes), info (and V, AtU with loadings)"""
    q0, us = [sh.vecN(q) for q in _q0(sh, cs, block)], [sh.vecN().fill(7.0) for _ in range(cs["k"])]
    vs = []
    try:
        ev, rs = sh.pca_dev(q0, us, tol, max_iter)
        out = dict(eval=ev, resid=rs, U=np.stack([u.download() for u in us]), info=sh.pca_info())
        assert all(np.array_equal(q.download(), w) for q, w in zip(q0, _q0(sh, cs, block)))         # q0 is not modified
        if loadings:
            vs = [sh.vecM().fill(7.0) for _ in us]
            sh.pca_loadings_dev(us, ev, vs)
            out["V"] = np.stack([v.download() for v in vs])
            w = sh.vecM()
            vs.append(w)
            out["AtU"] = []
            for u in us:
                sh.atx_dev(u, w)
                out["AtU"].append(w.download())
        return out
    finally:
        for v in q0 + us + vs:
            v.free()


def _baseline(name):
    """the default engine's result on a shape, computed once"""
    if name not in _RUNS:
        cs = pr.case(name)
        with _shard(cs) as sh:
            assert sh.get_layout() == 2 and sh.get_kernel_mode() == 1
            _RUNS[name] = _run(sh, cs, loadings=True)
    return _RUNS[name]


def _check(cs, res, tol=TOL, converged=True):
    N = cs["N"]
    assert np.all(res["U"][:, N:] == 0)                                                            # pad slots
    fig = pr.check_pairs(cs, res["eval"], res["U"][:, :N].T, res["resid"], tol, converged=converged)
    print(cs["name"], res["info"]["iterations"], fig)
    return fig


def _bits(res):
    return [np.asarray(res[k]).view(np.uint64) for k in ("U", "eval", "resid")]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ---- 1-3. the residual promise, the theorems, the structure ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_eigenpairs_hold_the_bounds_on_every_shape(name):
    cs = pr.case(name)
    res = _baseline(name)
    _check(cs, res)
    info = res["info"]
    ref = pr.iterate(cs, TOL, MAX_ITER)
    assert info["converged"] == 1 and info["iterations"] <= ref["iterations"] + 2, (info, ref["iterations"])
    assert info["block"] == cs["L"] and info["cols_atxm"] == info["cols_score"] == cs["L"] * info["iterations"]
    assert info["scratch_bytes"] >= 4 * cs["L"] * 4 * ((cs["N"] + 3) // 4) * 8


# ---- 4. bit reproducibility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "second-step", "many"])
def test_the_same_call_twice_gives_the_same_bits(name):
    cs = pr.case(name)
    with _shard(cs) as sh:
        a, b = _run(sh, cs), _run(sh, cs)
    assert _same_bits(a, b) and _same_bits(a, _baseline(name))


@pytest.mark.parametrize("pin", list(PINS))
@pytest.mark.parametrize("name", ["ragged", "second-step", "many"])
def test_the_products_pins_do_not_move_a_bit(name, pin):
    cs = pr.case(name)
    with _shard(cs, env=PINS[pin]) as sh:
        if pin == "forced-multi":
            sh.force_multi(1)
        res = _run(sh, cs)
        if pin == "no-kernels":
            assert sh.atxm_info()["path"] == "fallback" and sh.score_info()["path"] == "fallback"
    assert _same_bits(res, _baseline(name)), pin
    assert res["info"]["iterations"] == _baseline(name)["info"]["iterations"]


# ---- 5. other engines ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ["second-step", "ragged", "wide"])
def test_other_engines_hold_the_same_properties(name, engine):
    cs = pr.case(name)
    with _shard(cs, **ENGINES[engine]) as sh:
        res = _run(sh, cs)
    _check(cs, res)
    assert res["info"]["converged"] == 1 and res["info"]["iterations"] <= pr.iterate(cs, TOL, MAX_ITER)["iterations"] + 2


def test_dosage_codes_hold_the_residual_promise_by_the_contexts_own_products():
    """8-bit dosage codes, 257 x 65: synth_dosage's codes halved plus 80 codes at the individuals of one of three populations, the
    population drawn per marker.  The residual is formed with gv_ax / gv_atx of the same context: r = (N / M) A (A^T u) - theta u"""
    N, M, k, L = 257, 65, 2, 8
    rng = np.random.default_rng(211)
    pop, grp = np.arange(N) % 3, rng.integers(0, 3, M)
    codes = (synth.synth_dosage(N, M, 5, 8).reshape(M, N) // 2 + 80 * (pop[None, :] == grp[:, None])).astype(np.uint8)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(codes, 1.0 / 127)
        sh.set_mask(pr.mask4(np.ones(N, dtype=bool)), N)
        sh.compute_markers_statistics()
        Q = np.zeros((L, 4 * sh.mbytes))
        Q[:, :N] = rng.standard_normal((L, N))
        q0, us = [sh.vecN(q) for q in Q], [sh.vecN() for _ in range(k)]
        ev, rs = sh.pca_dev(q0, us, TOL, MAX_ITER)
        info = sh.pca_info()
        assert info["converged"] == 1
        for i in range(k):
            u = us[i].download()
            r = (N / M) * sh.Ax(sh.ATx(u)) - ev[i] * u
            out = float(np.sqrt((r * r).sum()))
            print("dosage", i, ev[i], rs[i], out, info["iterations"])
            assert out <= 1.01 * TOL * ev[i] and abs(rs[i] - out) <= 0.01 * out
            assert abs(float(u @ u) - 1.0) <= N * pr.EPS and u[int(np.argmax(np.abs(u)))] > 0
        assert ev[0] >= ev[1] > 0


# ---- 6. loadings --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_loadings_are_one_rounding_after_the_product(name):
    cs = pr.case(name)
    res = _baseline(name)
    N, M = cs["N"], cs["M"]
    for i in range(cs["k"]):
        c = np.sqrt(np.float64(N) / np.float64(M)) / np.sqrt(np.float64(res["eval"][i]))
        want = c * res["AtU"][i]
        assert np.array_equal(res["V"][i].view(np.uint64), want.view(np.uint64)), i
        assert abs(float(res["V"][i] @ res["V"][i]) - 1.0) < 1e-6          # a right singular vector (to the residual's order)


def test_shard_pca_draws_its_block_and_reports(monkeypatch):
    cs = pr.case("ragged")
    with _shard(cs) as sh:
        out = sh.pca(2, tol=TOL, loadings=True)
        assert out["evec"].shape == (2, cs["N"]) and out["loadings"].shape == (2, cs["M"]) and out["info"]["block"] == 10
        _check(cs, dict(eval=out["eval"], resid=out["resid"], U=out["evec"], info=out["info"]))
        block = np.random.default_rng(0).standard_normal((10, cs["N"]))
        same = _run(sh, dict(cs, L=10), block=block)
        assert np.array_equal(same["U"][:, :cs["N"]].view(np.uint64), out["evec"].view(np.uint64))
        with pytest.raises(capi.GvError, match="not converged after 1 iterations"):
            sh.pca(2, tol=TOL, max_iter=1)
        loose = sh.pca(2, tol=TOL, max_iter=1, strict=False)
        assert loose["info"]["converged"] == 0
        with pytest.raises(capi.GvError, match="block"):
            sh.pca(2, block=33)


# ---- 7. the context as found -------------------------------------------------------------------------------------------------------------
def test_a_pca_call_leaves_the_context_as_it_found_it():
    cs = pr.case("ragged")
    rng = np.random.default_rng(17)
    with _shard(cs) as sh:
        xa, pa = rng.standard_normal(cs["M"]), np.zeros(4 * sh.mbytes)
        pa[:cs["N"]] = rng.standard_normal(cs["N"]) * cs["present"]
        W = rng.standard_normal((5, cs["M"]))
        P = np.tile(pa, (5, 1)) * np.arange(1, 6)[:, None]

        def probe():
            x, p, zn, zm = sh.vecM(xa), sh.vecN(pa), sh.vecN(), sh.vecM()
            ws, zs = [sh.vecM(w) for w in W], [sh.vecN() for _ in W]
            ps, os_ = [sh.vecN(q) for q in P], [sh.vecM() for _ in P]
            out = []
            sh.ax_dev(x, zn)
            out.append(zn.download())
            sh.atx_dev(p, zm)
            out.append(zm.download())
            sh.lmmse_mult(x, 1.3, 0.4, zm)
            out.append(zm.download())
            sh.score_dev(ws, zs)
            out += [z.download() for z in zs]
            sh.atxm_dev(ps, os_)
            out += [o.download() for o in os_]
            for v in [x, p, zn, zm] + ws + zs + ps + os_:
                v.free()
            return [sh.decomp()] + out

        before = probe()
        res = _run(sh, cs)
        after = probe()
        assert before[0] == after[0]
        for a, b in zip(before[1:], after[1:]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert _same_bits(res, _baseline("ragged"))          # (and the probes before it did not move the result)


# ---- 8. edges -------------------------------------------------------------------------------------------------------------------------------
def _raw(sh, k, L, q0, tol, max_iter, us, ev=True, rs=True):
    """gv_pca_dev with every argument as given: (message or None, eval, resid)"""
    e, r = np.full(40, np.nan), np.full(40, np.nan)
    rc = sh.L.gv_pca_dev(sh.h, k, L, sh._handles(q0), tol, max_iter, sh._handles(us), capi._dp(e) if ev else None, capi._dp(r) if rs else None)
    return (sh.L.gv_last_error(sh.h).decode() if rc else None), e, r


def test_refusals_come_by_message_and_write_nothing():
    cs = pr.case("second-step")
    k, L = cs["k"], cs["L"]
    with _shard(cs) as sh, _shard(cs) as other:
        q0, us = [sh.vecN(q) for q in _q0(sh, cs)], [sh.vecN().fill(7.0) for _ in range(k)]
        m, foreign = sh.vecM(), other.vecN()
        cases = [
            ("k must be at least 1", (0, L, q0, TOL, 5, us)),
            ("block L must be at least k", (2, 1, q0[:1], TOL, 5, us)),
            ("above GV_PCA_MAX_BLOCK", (2, 33, q0 * 5, TOL, 5, us)),
            ("tol must be a positive finite number", (k, L, q0, 0.0, 5, us)),
            ("tol must be a positive finite number", (k, L, q0, -1e-9, 5, us)),
            ("tol must be a positive finite number", (k, L, q0, float("nan"), 5, us)),
            ("tol must be a positive finite number", (k, L, q0, float("inf"), 5, us)),
            ("max_iter must be at least 1", (k, L, q0, TOL, 0, us)),
            ("is NULL", (k, L, None, TOL, 5, us)),
            ("is NULL", (k, L, q0, TOL, 5, None)),
            (r"q0\[3\] is NULL", (k, L, q0[:3] + [None] + q0[4:], TOL, 5, us)),
            (r"u\[1\] is NULL", (k, L, q0, TOL, 5, [us[0], None])),
            ("column 1: u must be N-space", (k, L, q0, TOL, 5, [us[0], m])),
            ("column 2: q0 must be N-space", (k, L, q0[:2] + [m] + q0[3:], TOL, 5, us)),
            ("column 1: two outputs are the same vector", (k, L, q0, TOL, 5, [us[0], us[0]])),
            ("column 4: an output is also an input", (k, L, q0[:4] + [us[1]] + q0[5:], TOL, 5, us)),
            ("column 0: q0 belongs to another context", (k, L, [foreign] + q0[1:], TOL, 5, us)),
        ]
        for msg, args in cases:
            got, e, r = _raw(sh, *args)
            assert got is not None and __import__("re").search(msg, got), (msg, got)
            assert np.all(np.isnan(e)) and np.all(np.isnan(r)) and all(np.all(u.download() == 7.0) for u in us), msg
        assert _raw(sh, k, L, q0, TOL, 5, us, ev=False)[0] and _raw(sh, k, L, q0, TOL, 5, us, rs=False)[0]
        # a starting block with two equal columns: the Cholesky message
        twin = _q0(sh, cs)
        twin[5] = twin[2]
        tq = [sh.vecN(q) for q in twin]
        got, e, r = _raw(sh, k, L, tq, TOL, 5, us)
        assert got and "Cholesky pivot is not positive" in got, got
        assert np.all(np.isnan(e)) and all(np.all(u.download() == 7.0) for u in us)
        # the context still serves after every refusal
        assert _same_bits(_run(sh, cs), _baseline("second-step"))
    # the block above min(nonas, Mt)
    ts = pr.case("tile")
    with _shard(ts) as sh:
        q0, us = [sh.vecN().fill(1.0) for _ in range(4)], [sh.vecN().fill(7.0)]
        got, _, _ = _raw(sh, 1, 4, q0, TOL, 5, us)
        assert got and "above min(nonas, Mt) = 3" in got, got
    # marker statistics missing: the message of the products
    with _shard(cs, stats=False) as sh:
        q0, us = [sh.vecN(q) for q in _q0(sh, cs)], [sh.vecN().fill(7.0) for _ in range(k)]
        x, z = sh.vecM().fill(0.0), sh.vecN()
        with pytest.raises(capi.GvError) as single:
            sh.ax_dev(x, z)
        got, _, _ = _raw(sh, k, L, q0, TOL, 5, us)
        assert got == str(single.value) and "statistics" in got and all(np.all(u.download() == 7.0) for u in us)
    # vectors of earlier dimensions
    with _shard(cs) as sh:
        old = sh.vecN()
        sh.set_dims(cs["N"] + 256, cs["M"])
        q0, us = [sh.vecN() for _ in range(L)], [sh.vecN() for _ in range(k)]
        got, _, _ = _raw(sh, k, L, [old] + q0[1:], TOL, 5, us)
        assert got and "earlier dimensions" in got, got


def test_one_iteration_returns_unconverged_pairs_with_honest_residuals():
    cs = pr.case("ragged")
    with _shard(cs) as sh:
        res = _run(sh, cs, max_iter=1)
    assert res["info"]["converged"] == 0 and res["info"]["iterations"] == 1
    _check(cs, res, converged=False)
    assert np.all(res["resid"] > TOL * res["eval"])
