"""The LD-block preconditioner on 8-bit dosage codes (gv_set_ld_dosage + gv_set_cg_precond kind 1) on the GPU
against tests/precond_dosage_restatement.py: every window Gram of both grids from the one-product kernel, the forced four-product kernel
and a one-step segment cap; the apply, the CG solvers and the VAMP loop on gv_synth_dosage_ld's codes against the scalar rule and
tests/precond_restatement.py; the synthesiser against its host twin; the driver; the refusals; and the context left as it was."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, hostapi, synth
import ld_dosage_restatement as ldd
import precond_dosage_restatement as pdr
import precond_restatement as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 1.0 / 127.0


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mask4(na):
    m = np.zeros((na.size + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(codes, S=0, Mt=None, na=None, missing=False, W=128, forced4=False, seg=None, route=0):
    """a context with the codes resident, the statistics computed and kind 1 set; the development switches are read by gv_create, per
    context, and cleared again at once"""
    M, N = codes.shape
    env = {}
    if forced4:
        env["GV_DOSAGE_NA_KERNELS"] = 1
    if seg is not None:
        env["GV_DOSAGE_MFMA_SEG"] = seg
    with _env(**env):
        sh = capi.Shard(N, M, Mt=Mt if Mt is not None else S + M, S=S, device=0)
    sh.set_dosage_route(route)
    sh.upload_dosage(codes, SCALE, missing=missing or forced4)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    sh.compute_markers_statistics()
    sh.set_ld_dosage(1)
    sh.set_cg_precond("ld", W)
    return sh


def _grams(sh, wins):
    return {(g, k): sh.precond_window_gram(g, k) for g, k, _, _ in wins}


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def test_kind_1_is_accepted_on_8_bit_codes_under_the_option():
    """fails without the feature: gv_set_cg_precond(ctx, 1, W) refuses compact dosage data whatever gv_set_ld_dosage says"""
    N, M = 300, 200
    with capi.Shard(N, M, device=0) as sh:
        sh.synth_dosage(1, 8)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match=r"compact dosage data \(8-bit codes\)"):        # the default: today's refusal
            sh.set_cg_precond("ld", 64)
        sh.set_ld_dosage(1)
        sh.set_cg_precond("ld", 64)
        info = sh.precond_info()
        assert info["kind"] == 1 and info["window"] == 64
        G = sh.precond_window_gram(0, 0)
        assert G.shape == (64, 64) and np.all(np.isfinite(G)) and np.all(np.diag(G) > 0)
        info = sh.precond_info()
        assert info["build_seconds"] > 0 and info["resident_bytes"] == 2 * 8 * sum(info["windows"]) * 64 * 64


# (N, S, M, W): where the Gram epilogue of the block kernel can break
#   (1003, 0, 700, 128)    eleven row groups, a partly filled last one, N off the K-step
#   (1203, 37, 333, 64)    S off the row-group grid
#   (998, 5, 200, 32)      h = 16: several windows per row group and one across each edge
#   (5, 0, 3, 32)          a handful of entries; the second half of the only K-step lies past the row
#   (70, 0, 1, 64)         one marker, N below one K-step
#   (4099, 37, 130, 128)   S off the grid with W = 128: windows straddle three row groups, blocks (I, I + 2)
SHAPES = [(1003, 0, 700, 128), (1203, 37, 333, 64), (998, 5, 200, 32), (5, 0, 3, 32), (70, 0, 1, 64), (4099, 37, 130, 128)]
CASES = ("plain", "masked", "missing")


@functools.lru_cache(maxsize=None)
def _case(N, S, M, W, case):
    """(codes, na, missing, wins, reference Grams): computed once, shared and left unchanged.  plain and masked codes hold no 255 (the
    synthesiser clamps), so the same data serve the one-product kernel and the forced four-product kernel, which reads 255 as missing"""
    codes = synth.synth_dosage_ld(N, M, 3, 8, 48, 900000, miss_ppm=20000 if case == "missing" else 0, S=S)
    na = None
    if case != "plain":
        na = np.ones(N)
        na[::7] = 0.0
    missing = case == "missing"
    if not missing:
        assert not np.any(codes == 255)
    wins = pr.windows(S, M, W)
    ms = pdr.msig(codes, na, missing)
    ref = {(g, k): pdr.window_gram(codes, S, lo, hi, na, missing, ms=ms) for g, k, lo, hi in wins}
    return codes, na, missing, wins, ref


def _check_grams(got, wins, ref, W, tag):
    worst = 0.0
    for g, k, lo, hi in wins:
        G, R, n = got[(g, k)], ref[(g, k)], hi - lo
        assert G.shape == (W, W)
        assert np.all(G[n:, :] == 0) and np.all(G[:, n:] == 0), (tag, g, k)            # exact zeros beyond the clipped length
        assert np.array_equal(G, G.T), (tag, g, k)                                     # G_jk and G_kj are the same bits
        dmax = float(np.max(np.diag(R)))
        err = float(np.max(np.abs(G[:n, :n] - R)))
        worst = max(worst, err / dmax if dmax > 0 else err)
        assert err <= 1e-12 * dmax, (tag, g, k, err, dmax)
    print("max |G - ref| / max diag = %.3e" % worst, tag)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,S,M,W", SHAPES)
def test_every_window_gram_matches_the_restatement(N, S, M, W, case):
    codes, na, missing, wins, ref = _case(N, S, M, W, case)
    with _shard(codes, S, S + M + 100, na, missing, W) as sh:
        assert sh.dosage_info()["na_kernels"] == bool(np.any(codes == 255))
        first = _grams(sh, wins)
        _check_grams(first, wins, ref, W, (N, S, M, W, case))
        info = sh.precond_info()
        g0, g1 = [w for w in wins if w[0] == 0], [w for w in wins if w[0] == 1]
        assert info["windows"] == [len(g0), len(g1)] and info["first_window"] == [g0[0][1], g1[0][1]]
        assert info["build_seconds"] > 0 and info["resident_bytes"] == 2 * 8 * len(wins) * W * W
        assert _same(first, _grams(sh, wins))                                          # two calls
        sh.set_cg_precond("scalar", W)                                                 # releases the Grams
        sh.set_cg_precond("ld", W)
        assert _same(first, _grams(sh, wins))                                          # ... and builds the same bits again
    with _shard(codes, S, S + M + 100, na, missing, W, seg=128) as sh:                 # a one-step segment cap against the default
        assert _same(first, _grams(sh, wins))
    if not missing:                                                                    # the forced four-product path, no reserved code
        with _shard(codes, S, S + M + 100, na, False, W, forced4=True) as sh:
            assert sh.dosage_info()["na_kernels"] is True
            assert _same(first, _grams(sh, wins))
        with _shard(codes, S, S + M + 100, na, False, W, forced4=True, seg=128) as sh:
            assert _same(first, _grams(sh, wins))


@pytest.mark.parametrize("missing", [False, True])
def test_hand_placed_rows(missing):
    """rows at 63 / 64 (the row-group edge) and M - 1: constant, all missing, equal to and 255 - its neighbour"""
    N, S, M, W = 403, 0, 130, 128
    codes = synth.synth_dosage_ld(N, M, 5, 8, 48, 900000, miss_ppm=20000 if missing else 0).copy()
    na = np.ones(N)
    na[::5] = 0.0
    codes[63] = 253                              # constant: X_jj = 0 exactly
    codes[64] = 255 if missing else 7            # all missing (c_j = 0) / another constant
    codes[62] = codes[61]                        # equal to its neighbour
    codes[65] = 255 - codes[66]                  # 255 - its neighbour, across the edge from 63 / 64
    codes[M - 1] = 255 - codes[M - 2]
    codes[M - 3] = codes[M - 2]
    wins = pr.windows(S, M, W)
    ms = pdr.msig(codes, na, missing)
    ref = {(g, k): pdr.window_gram(codes, S, lo, hi, na, missing, ms=ms) for g, k, lo, hi in wins}
    with _shard(codes, S, M, na, missing, W) as sh:
        got = _grams(sh, wins)
    _check_grams(got, wins, ref, W, ("hand-placed", missing))
    G = got[(0, 0)]                              # grid 0, window 0 = markers [0, 128)
    assert G[63, 63] == 0.0 and G[64, 64] == 0.0
    assert np.all(G[64] == 0.0) and np.all(G[:, 64] == 0.0)
    if not missing:
        # complete rows.  A copy has its neighbour's statistics and integers: the same bits.  A mirror image has X negated exactly and
        # its own msig, which agrees with its neighbour's to rounding
        assert np.array_equal(G[62, :61], G[61, :61]) and G[62, 62] == G[61, 61] == G[61, 62]
        assert np.isclose(G[65, 66], -G[66, 66], rtol=1e-13, atol=0) and np.isclose(G[65, 65], G[66, 66], rtol=1e-13, atol=0)


@functools.lru_cache(maxsize=None)
def _bound():
    codes = ldd.bound_case()
    M = codes.shape[0]
    wins = pr.windows(0, M, 128)
    full = pdr.gram(codes)                       # M = 70 markers: every window is a diagonal block of the one Gram
    return codes, wins, {(g, k): full[lo:hi, lo:hi] for g, k, lo, hi in wins}


def test_the_int32_bound():
    """N = 140 000 > 131 071: the segmented instantiation at the default cap; tests/test_ld_dosage_cpu.py shows that rows 0 and 1 wrap
    an unsegmented int32 sum (VV_00 = 2 275 910 000, VV_01 = -2 275 840 000)"""
    codes, wins, ref = _bound()
    with _shard(codes) as sh:
        got = _grams(sh, wins)
    _check_grams(got, wins, ref, 128, "bound")
    G = got[(1, 0)]
    assert G[0, 0] > 0 and np.isclose(G[0, 1], -G[0, 0], rtol=1e-13, atol=0) and np.isclose(G[1, 1], G[0, 0], rtol=1e-13, atol=0)
    with _shard(codes, seg=128) as sh:
        assert _same(got, _grams(sh, wins))


# ---- apply and solvers on block-correlated codes ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ld_problem(N=3000, M=2048, ld_block=64):
    codes = synth.synth_dosage_ld(N, M, 77, 8, ld_block, 900000)
    return codes, np.asarray(pdr.matrix(codes, dtype=np.float64))


@pytest.mark.parametrize("route", [0, 1])
def test_apply_matches_restatement(route):
    N, M, S, W = 1500, 500, 37, 64
    codes = synth.synth_dosage_ld(N, M, 8, 8, 64, 900000, S=S)
    A = np.asarray(pdr.matrix(codes, dtype=np.float64))
    r = np.random.default_rng(2).standard_normal(M)
    with _shard(codes, S, W=W, route=route) as sh:
        assert sh.dosage_route()[1] == route
        dr, dz = sh.vecM(r), sh.vecM()
        for tau, gam2 in ((2.0, 0.05), (0.7, 3.0)):
            sh.precond_apply(tau, gam2, dr, dz)
            ref = pr.TwoGrid(A, S, W, tau, gam2)(r)
            assert np.linalg.norm(dz.download() - ref) <= 1e-12 * np.linalg.norm(ref)
        info = sh.precond_info()
        assert info["factorisations"] == 2 and info["fallback_windows"] == 0
        assert (info["last_tau"], info["last_gam2"]) == (0.7, 3.0)


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("denoiser", [1, 0])
def test_cg_solve_steps_and_solution_match_restatement(denoiser, route):
    N, M, W, tau = 3000, 2048, 128, 2.0
    codes, A = _ld_problem(N, M)
    v = np.random.default_rng(1).standard_normal(M)
    with _shard(codes, W=W, route=route) as sh:
        for gam2 in (0.05, 0.5):
            pc = pr.TwoGrid(A, 0, W, tau, gam2)
            mu_ref, steps, ok = pr.pcg(A, v, tau, gam2, denoiser, 500, pc)
            dv, dmu = sh.vecM(v), sh.vecM()
            sh.set_cg_precond("ld", W)
            st, rr = sh.cg_solve(dv, None, tau, gam2, denoiser, 500, dmu)
            assert ok and st.converged == 1 and st.iters == steps, (gam2, st.iters, steps)
            mu = dmu.download()
            assert np.linalg.norm(mu - mu_ref) <= 1e-9 * np.linalg.norm(mu_ref)
            if denoiser == 1:
                assert rr[-1] < 1e-5
                res = v - (tau * (A.T @ (A @ mu)) + gam2 * mu)
                assert np.linalg.norm(res) / np.linalg.norm(v) < 1.1e-5
            sh.set_cg_precond("scalar", W)
            ds = sh.vecM()
            ss, _ = sh.cg_solve(dv, None, tau, gam2, denoiser, 500, ds)
            print("gam2 %g denoiser %d route %d: scalar %d -> ld %d steps" % (gam2, denoiser, route, ss.iters, st.iters))
            assert ss.converged == 1 and 2 * st.iters <= ss.iters, (gam2, ss.iters, st.iters)


# ---- VAMP -------------------------------------------------------------------------------------------------------------------------
PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]
KW = dict(iterations=6, CG_max_iter=400, rho=0.5, seed=9, gam1=1e-8, gamw=2.0, stop_criteria_thr=1e-12)


def _passes(r, first=1):
    return sum(t["n_ax_pass"] + t["n_atx_pass"] for t in r.trace[first:])


def test_linear_vamp_on_ld_dosage_codes_against_the_scalar_run():
    N, M = 2000, 5000
    rng = np.random.default_rng(6)
    beta = rng.standard_normal(M) * (rng.random(M) < 0.02) * 0.15
    with capi.Shard(N, M) as sh:
        sh.synth_dosage_ld(77, 8, 64, 900000)
        sh.compute_markers_statistics()
        g = sh.Ax(beta * np.sqrt(N))[:N]
        raw = g + np.std(g) * rng.standard_normal(N)
        y = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))
        scalar = {f: hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, fuse_solves=f, **KW) for f in (1, 4)}
        with pytest.raises(capi.GvError, match="compact dosage data"):                 # without the option: the refusal of before
            hostapi.infere_linear(sh, y, PROBS, VARS, fuse_solves=4, cg_precond="ld", **KW)
        sh.set_ld_dosage(1)
        runs = {f: hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, fuse_solves=f, cg_precond="ld", **KW) for f in (0, 1, 4)}
        assert sh.precond_info()["kind"] == 1
    ref = scalar[1]
    assert all(t["cg_iters"] < KW["CG_max_iter"] and t["onsager_iters"] < KW["CG_max_iter"] for t in ref.trace + scalar[4].trace)
    for f, r in runs.items():
        assert r.niter == ref.niter
        for it in range(r.niter):
            assert rel(r.x1[it], ref.x1[it]) < 1e-4, (f, it, rel(r.x1[it], ref.x1[it]))
        assert all(t["probe_product"] == 0 for t in r.trace), f
    assert all(np.array_equal(runs[1].x1[it], runs[0].x1[it]) for it in range(KW["iterations"]))
    print("level-4 passes over iterations 2-6: scalar %d, ld %d (ratio %.3f); CG / Onsager steps scalar %s, ld %s" %
          (_passes(scalar[4]), _passes(runs[4]), _passes(runs[4]) / _passes(scalar[4]),
           [(t["cg_iters"], t["onsager_iters"]) for t in scalar[4].trace], [(t["cg_iters"], t["onsager_iters"]) for t in runs[4].trace]))
    assert _passes(runs[4]) < _passes(scalar[4]), (_passes(runs[4]), _passes(scalar[4]))


# ---- the synthesiser --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,miss_ppm", [(8, 0), (8, 30000), (16, 0), (16, 30000)])
def test_device_synthesiser_equals_the_host_twin(bits, miss_ppm):
    """gv_synth_dosage_ld at a shard offset against synth.synth_dosage_ld: the same reserved-code count, identical statistics and
    products, and EVERY code read back through ATx of unit vectors (column n of all rows per call)"""
    N, Mt, S, M, seed = 203, 400, 117, 150, 99
    scale = 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0
    res = (1 << bits) - 1
    twin = synth.synth_dosage_ld(N, Mt, seed, bits, 48, 900000, miss_ppm=miss_ppm)[S:S + M]
    assert np.array_equal(twin, synth.synth_dosage_ld(N, M, seed, bits, 48, 900000, miss_ppm=miss_ppm, S=S))
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    outs = []
    for how in ("array", "synth"):
        with capi.Shard(N, M, Mt=Mt, S=S) as sh:
            if how == "array":
                sh.upload_dosage(twin, scale, missing=miss_ppm > 0)
            else:
                sh.synth_dosage_ld(seed, bits, 48, 900000, miss_ppm=miss_ppm)
            info = sh.dosage_info()
            assert info == dict(bits=bits, scale=scale, missing=miss_ppm > 0, reserved=int((twin == res).sum()),
                                na_kernels=miss_ppm > 0), (how, info)
            sh.compute_markers_statistics()
            mave, msig = sh.marker_stats()
            outs.append((mave, msig, sh.Ax(x), sh.ATx(p)))
            if how == "synth":
                got = np.empty((M, N))
                e = np.zeros(p.size)
                for n in range(N):
                    e[n] = 1.0
                    got[:, n] = sh.ATx(e)
                    e[n] = 0.0
                back = got * np.sqrt(N) / (msig * scale)[:, None] + (mave / scale)[:, None]
                keep = twin != res if miss_ppm else np.ones(twin.shape, dtype=bool)
                assert np.array_equal(np.rint(back[keep]).astype(np.int64), twin[keep].astype(np.int64))
                assert np.all(got[~keep] == 0.0)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert (miss_ppm > 0) == bool(np.any(twin == res))


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def test_gvamp_main_real_with_the_ld_preconditioner_on_a_dosage8_file_equals_the_host_api_run(tmp_path):
    N, Mt, it = 600, 1500, 3
    B = synth.synth_dosage_ld(N, Mt, 41, 8, 64, 900000)
    cfile, pfile = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen")
    B.tofile(cfile)
    rng = np.random.default_rng(6)
    beta = rng.standard_normal(Mt) * (rng.random(Mt) < 0.05) * 0.15
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(B, SCALE)
        sh.compute_markers_statistics()
        g = sh.Ax(beta * np.sqrt(N))[:N]
    raw = 1.5 + 2.0 * (g + 0.7 * rng.standard_normal(N))
    with open(pfile, "w") as f:
        for i in range(N):
            f.write("F%d I%d %s\n" % (i, i, repr(float(raw[i]))))
    out = str(tmp_path / "out") + "/"
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    base = [exe, "--run-mode", "infere", "--bed-file", cfile, "--phen-files", pfile, "--N", str(N), "--Mt", str(Mt), "--out-dir", out,
            "--out-name", "d", "--iterations", str(it), "--probs", "0.9,0.1", "--vars", "0,0.01", "--rho", "0.5", "--CG-max-iter", "60",
            "--seed", "4", "--cg-precond", "ld", "--cg-precond-window", "64"]
    res = subprocess.run(base + ["--geno-format", "dosage8", "--ld-dosage", "1"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    x_drv = np.fromfile(out + "d_it_%d.bin" % it)
    y = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))          # data::read_phen
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage_file(cfile, 8, SCALE)
        sh.set_ld_dosage(1)
        r = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], iterations=it, CG_max_iter=60, rho=0.5, seed=4, gam1=1e-6, gamw=2.0,
                                  fuse_solves=4, cg_precond="ld", cg_precond_window=64)
        s = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], iterations=it, CG_max_iter=60, rho=0.5, seed=4, gam1=1e-6, gamw=2.0,
                                  fuse_solves=4)
    print("driver vs host API rel %.3e; ld vs scalar rel %.3e" % (rel(r.x1[it - 1], x_drv), rel(r.x1[it - 1], s.x1[it - 1])))
    assert rel(r.x1[it - 1], x_drv) < 1e-9
    assert np.all(np.isfinite(x_drv)) and np.any(x_drv != 0)
    assert not np.array_equal(r.x1[it - 1], s.x1[it - 1])                 # the preconditioner did run
    # without the flag the FATAL line of before; dosage16 with it names the width
    for extra, msg in ((["--geno-format", "dosage8"], "--cg-precond ld is not available for compact dosage data"),
                       (["--geno-format", "dosage8", "--ld-dosage", "0"], "--cg-precond ld is not available for compact dosage data"),
                       (["--geno-format", "dosage16", "--ld-dosage", "1"], "dosage16")):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode != 0 and "FATAL" in res.stdout and msg in res.stdout, res.stdout[-2000:]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    N, M = 600, 256
    codes = synth.synth_dosage_ld(N, M, 2, 8, 32, 900000)
    with capi.Shard(N, M, device=0) as sh:              # 16-bit codes
        sh.set_ld_dosage(1)
        sh.upload_dosage(synth.synth_dosage(N, M, 2, 16), 1.0 / 16384.0)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="16-bit codes"):
            sh.set_cg_precond("ld", 64)
    with capi.Shard(N, M, device=0) as sh:              # methylation data
        sh.set_ld_dosage(1)
        sh.synth_meth(3)
        with pytest.raises(capi.GvError, match="meth"):
            sh.set_cg_precond("ld", 64)
    with capi.Shard(N, M, device=0) as sh:              # statistics not computed
        sh.upload_dosage(codes, SCALE)
        sh.set_ld_dosage(1)
        sh.set_cg_precond("ld", 64)
        with pytest.raises(capi.GvError, match="marker statistics must be computed first"):
            sh.precond_window_gram(0, 0)
    with _shard(codes, W=64) as sh:
        with pytest.raises(capi.GvError, match="window must be 32, 64 or 128"):
            sh.set_cg_precond("ld", 96)
        vn, mn = sh.vecN(np.ones(4 * sh.mbytes)), sh.vecN()          # the N-space solver
        with pytest.raises(capi.GvError, match="N-space solver"):
            sh.cg_solve_aat(vn, None, 1.0, 1.0, 10, mn)
        va, vb, ma, mb, at = sh.vecM(np.ones(M)), sh.vecM(np.arange(M) % 3 - 1.0), sh.vecM(), sh.vecM(), sh.vecM()
        with pytest.raises(capi.GvError, match="ata_v_b"):            # gv_cg_warm::ata_v_b under kind 1
            sh.cg_solve2x(va, None, vb, 1.0, 1.0, 10, ma, mb, ata_v_b=at)
        sh.cg_solve2(va, None, vb, 1.0, 1.0, 10, ma, mb)             # ... and without it the two-system solve runs
        # kind 1 accepted, then the option switched off: the next Gram read, apply and solve refuse, naming the option
        sh.set_ld_dosage(0)
        for call in (lambda: sh.precond_window_gram(0, 0), lambda: sh.precond_apply(1.0, 1.0, va, ma),
                     lambda: sh.cg_solve(va, None, 1.0, 1.0, 1, 10, ma)):
            with pytest.raises(capi.GvError, match="gv_set_ld_dosage") as ei:
                call()
            assert "compact dosage data (8-bit codes)" in str(ei.value)
        sh.set_cg_precond("scalar", 64)                              # the scalar rule stays available
        sh.cg_solve(va, None, 1.0, 1.0, 1, 10, ma)
        with pytest.raises(capi.GvError, match=r"compact dosage data \(8-bit codes\)"):
            sh.set_cg_precond("ld", 64)
        sh.set_ld_dosage(1)
        sh.set_cg_precond("ld", 64)
        sh.cg_solve(va, None, 1.0, 1.0, 1, 10, ma)


def test_the_grams_follow_the_data_the_mask_and_the_options():
    """dropped by a new upload or synthesis, gv_set_mask, gv_marker_stats and gv_set_ld_dosage"""
    N, M, W = 403, 130, 64
    a = synth.synth_dosage_ld(N, M, 5, 8, 48, 900000)
    b = synth.synth_dosage_ld(N, M, 6, 8, 48, 900000, miss_ppm=20000)
    wins = pr.windows(0, M, W)
    na = np.ones(N)
    na[::3] = 0.0

    def ref(codes, na=None, missing=False):
        ms = pdr.msig(codes, na, missing)
        return {(g, k): pdr.window_gram(codes, 0, lo, hi, na, missing, ms=ms) for g, k, lo, hi in wins}

    with _shard(a, W=W, missing=True) as sh:                         # (a holds no 255; the setting cannot change under resident codes)
        _check_grams(_grams(sh, wins), wins, ref(a, None, True), W, "first")
        sh.upload_dosage(b, SCALE, missing=True)                     # a new upload
        sh.compute_markers_statistics()
        _check_grams(_grams(sh, wins), wins, ref(b, None, True), W, "upload")
        sh.set_mask(_mask4(na), int(na.sum()))
        sh.compute_markers_statistics()
        _check_grams(_grams(sh, wins), wins, ref(b, na, True), W, "mask")
        sh.synth_dosage_ld(5, 8, 48, 900000)                         # a synthesis (the mask stays)
        sh.compute_markers_statistics()
        g = _grams(sh, wins)
        _check_grams(g, wins, ref(a, na, True), W, "synth")
        sh.set_ld_dosage(0)
        sh.set_ld_dosage(1)
        assert sh.precond_info()["build_seconds"] > 0 and _same(g, _grams(sh, wins))


@pytest.mark.parametrize("case", ["masked", "missing"])
def test_the_context_is_left_as_it_was(case):
    """Ax, ATx, assoc_calc, ld_scores and ld_band give the same bits before and after a Gram build and a preconditioned solve"""
    N, S, M, W = 1003, 0, 700, 128
    codes, na, missing, wins, _ = _case(N, S, M, W, case)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    M_, N_ = codes.shape
    with capi.Shard(N_, M_, device=0) as sh:
        sh.upload_dosage(codes, SCALE, missing=missing)
        sh.set_mask(_mask4(na), int(na.sum()))
        sh.compute_markers_statistics()
        sh.set_ld_dosage(1)

        def outputs():
            z = sh.Ax(x)
            w = sh.ATx(z)
            y = np.zeros(z.size)
            y[:N] = np.random.default_rng(2).standard_normal(N)
            loo = sh.assoc_calc(sh.vecN(z), sh.vecN(y), sh.vecM(x))
            return [z, w] + [loo[k] for k in ("beta", "se", "t", "p")] + list(sh.ld_scores(100)) + [sh.ld_band(100, 10, 50)]

        before, ld_info = outputs(), sh.ld_info()
        sh.set_cg_precond("ld", W)
        sh.precond_window_gram(0, 0)
        assert sh.ld_info() == ld_info                                # gv_ld_info still describes the last LD call
        dv, dmu = sh.vecM(x), sh.vecM()
        st, _ = sh.cg_solve(dv, None, 2.0, 0.5, 1, 200, dmu)
        assert st.converged == 1
        after = outputs()
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(before, after))
        sh.set_cg_precond("scalar", W)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(before, outputs()))
