"""The LD-block preconditioner on the GPU (gv_set_cg_precond kind 1) against the numpy restatement of
tests/precond_restatement.py: window Grams on both layouts and both MFMA kernel modes, the two-grid apply and its scalar fallback,
the CG solvers' step counts and solutions, reproducibility and the refusals."""
import numpy as np
import pytest

from gvamp_amd import capi, synth
import precond_restatement as pr

pytestmark = pytest.mark.gpu


def _mask4(na):
    N = na.size
    m = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(bed, N, M, S=0, Mt=None, layout=2, mode=1, na=None, W=128):
    sh = capi.Shard(N, M, Mt=Mt if Mt is not None else S + M, S=S, device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(bed)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    sh.compute_markers_statistics()
    sh.set_cg_precond("ld", W)
    return sh


def _host(bed, N, M, S, na=None):
    a, b = pr.decode(bed, N, M)
    na = np.ones(N) if na is None else na
    mave, msig = pr.marker_stats(a, b, na)
    return a, b, na, mave, msig


# The Grams are an epilogue of the LD block kernel (64-marker row groups, K-blocks of 256 individuals).  After the three larger
# shapes, the smallest at which that epilogue can go wrong:
#   (100, 0, 40, 128)    one row group, one K-block whose second half is all mask-zero, a window longer than the shard
#   (257, 64, 130, 128)  the shard offset on a row-group and window edge, a partly filled last row group, one individual in the
#                        second K-block
#   (300, 37, 200, 128)  windows that straddle three row groups: blocks (I, I + 2)
#   (300, 5, 70, 32)     h = 16: several windows per row group and one across the edge at local marker 64
#   (130, 3, 1, 64)      a single marker
@pytest.mark.parametrize("N,S,M,W,masked", [(2001, 37, 650, 128, False), (1203, 37, 333, 64, True), (998, 5, 200, 32, False),
                                            (100, 0, 40, 128, False), (257, 64, 130, 128, True), (300, 37, 200, 128, False),
                                            (300, 5, 70, 32, False), (130, 3, 1, 64, False)])
def test_window_grams_match_restatement_on_both_layouts_and_modes(N, S, M, W, masked):
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000)
    na = None
    if masked:
        na = np.ones(N)
        na[::7] = 0.0
    a, b, na_h, mave, msig = _host(bed, N, M, S, na)
    wins = pr.windows(S, M, W)
    grams = {}
    for layout, mode in ((2, 1), (1, 1), (2, 2)):
        with _shard(bed, N, M, S=S, Mt=S + M + 100, layout=layout, mode=mode, na=na, W=W) as sh:
            info = sh.precond_info()
            assert info["kind"] == 1 and info["window"] == W
            for grid, k, lo, hi in wins:
                G = sh.precond_window_gram(grid, k)
                n = hi - lo
                ref = pr.gram_planes(a, b, na_h, mave, msig, S, lo, hi)
                assert np.all(G[n:, :] == 0) and np.all(G[:, n:] == 0)
                assert np.max(np.abs(G[:n, :n] - ref)) <= 1e-12 * np.max(np.diag(ref)), (layout, mode, grid, k)
                grams.setdefault((grid, k), []).append(G)
            info = sh.precond_info()          # (after the first Gram read has built them)
            g0 = [w for w in wins if w[0] == 0]
            g1 = [w for w in wins if w[0] == 1]
            assert info["windows"] == [len(g0), len(g1)]
            assert info["first_window"] == [g0[0][1], g1[0][1]]
            assert info["build_seconds"] > 0 and info["resident_bytes"] == 2 * 8 * len(wins) * W * W
    for key, gs in grams.items():      # layouts and kernel modes agree bit for bit
        assert all(np.array_equal(gs[0], g) for g in gs[1:]), key


def test_ld_band_and_window_grams_give_the_same_correlations():
    """the two users of the block kernel: r_jk of gv_ld_band against G_jk / sqrt(G_jj G_kk) of every window that holds both markers.
    Both are held to 1e-12 against the same restatement and the diagonal of r is 1, hence 1e-12."""
    N, S, M, W = 300, 37, 200, 128
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000)
    with _shard(bed, N, M, S=S, W=W) as sh:
        r = sh.ld_band(W, 0, M)
        pairs = 0
        for grid, k, lo, hi in pr.windows(S, M, W):
            n, j0 = hi - lo, lo - S
            G = sh.precond_window_gram(grid, k)[:n, :n]
            d = np.diag(G)
            poly = d != 0
            assert poly.sum() >= 2
            jj, kk = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            rb = r[j0 + jj, W + kk - jj]
            rg = G / np.sqrt(np.outer(d, d), where=np.outer(poly, poly), out=np.ones((n, n)))
            both = np.outer(poly, poly)
            assert np.max(np.abs(rb - rg)[both]) <= 1e-12, (grid, k)
            pairs += int(both.sum())
        assert pairs > M * W // 2


def test_apply_matches_restatement_and_counts_singular_windows():
    N, M, S, W = 1500, 500, 37, 64
    bed = synth.synth_bed(N, M, seed=8, miss_ppm=5000, S=S, ld_block=64, ld_ppm=900000)
    a, b, na, mave, msig = _host(bed, N, M, S)
    A = pr.matrix(a, b, na, mave, msig)
    r = np.random.default_rng(2).standard_normal(M)
    with _shard(bed, N, M, S=S, W=W) as sh:
        dr, dz = sh.vecM(r), sh.vecM()
        for tau, gam2 in ((2.0, 0.05), (0.7, 3.0)):
            sh.precond_apply(tau, gam2, dr, dz)
            ref = pr.TwoGrid(A, S, W, tau, gam2)(r)
            assert np.linalg.norm(dz.download() - ref) <= 1e-12 * np.linalg.norm(ref)
        info = sh.precond_info()
        assert info["factorisations"] == 2 and info["fallback_windows"] == 0
        assert (info["last_tau"], info["last_gam2"]) == (0.7, 3.0)
    # duplicated markers and gam2 = 0: the windows holding both copies are singular and take the scalar rule
    mb = (N + 3) // 4
    bed2 = np.array(synth.synth_bed(N, M, seed=9, miss_ppm=5000, S=S), dtype=np.uint8).reshape(M, mb).copy()
    bed2[101] = bed2[100]
    a, b, na, mave, msig = _host(bed2.ravel(), N, M, S)
    A = pr.matrix(a, b, na, mave, msig)
    ref_pc = pr.TwoGrid(A, S, W, 1.0, 0.0)
    assert ref_pc.fallback == 2
    with _shard(bed2.ravel(), N, M, S=S, W=W) as sh:
        dr, dz = sh.vecM(r), sh.vecM()
        sh.precond_apply(1.0, 0.0, dr, dz)
        assert sh.precond_info()["fallback_windows"] == 2
        ref = ref_pc(r)
        assert np.linalg.norm(dz.download() - ref) <= 1e-10 * np.linalg.norm(ref)


def _ld_problem(N=3000, M=2048, ld_block=64):
    bed = synth.synth_bed(N, M, seed=77, miss_ppm=5000, ld_block=ld_block, ld_ppm=900000)
    a, b, na, mave, msig = _host(bed, N, M, 0)
    return bed, pr.matrix(a, b, na, mave, msig)


@pytest.mark.parametrize("denoiser", [1, 0])
def test_cg_solve_steps_and_solution_match_restatement(denoiser):
    N, M, W, tau = 3000, 2048, 128, 2.0
    bed, A = _ld_problem(N, M)
    v = np.random.default_rng(1).standard_normal(M)
    with _shard(bed, N, M, W=W) as sh:
        for gam2 in (0.05, 0.5):
            pc = pr.TwoGrid(A, 0, W, tau, gam2)
            mu_ref, steps, ok = pr.pcg(A, v, tau, gam2, denoiser, 500, pc)
            dv, dmu = sh.vecM(v), sh.vecM()
            st, rr = sh.cg_solve(dv, None, tau, gam2, denoiser, 500, dmu)
            assert ok and st.converged == 1 and st.iters == steps, (gam2, st.iters, steps)
            mu = dmu.download()
            assert np.linalg.norm(mu - mu_ref) <= 1e-9 * np.linalg.norm(mu_ref)
            if denoiser == 1:
                assert rr[-1] < 1e-5
                res = v - (tau * (A.T @ (A @ mu)) + gam2 * mu)
                assert np.linalg.norm(res) / np.linalg.norm(v) < 1.1e-5


def test_two_system_solve_fewer_passes_same_solution():
    N, M, W, tau, gam2 = 3000, 2048, 128, 2.0, 0.3
    bed, A = _ld_problem(N, M, ld_block=48)
    rng = np.random.default_rng(4)
    va, vb = rng.standard_normal(M), rng.standard_normal(M)
    out = {}
    for kind in ("scalar", "ld"):
        with _shard(bed, N, M, W=W) as sh:
            sh.set_cg_precond(kind, W)
            dva, dvb, ma, mb = sh.vecM(va), sh.vecM(vb), sh.vecM(), sh.vecM()
            (sa, _), (sb, _) = sh.cg_solve2(dva, None, dvb, tau, gam2, 500, ma, mb)
            assert sa.converged == 1 and sb.converged == 1
            out[kind] = (ma.download(), mb.download(), sa.n_atx, sa.iters, sb.iters, sb.onsager)
    s, l = out["scalar"], out["ld"]
    assert np.linalg.norm(l[0] - s[0]) <= 1e-4 * np.linalg.norm(s[0])
    # the Onsager rule stops on the scalar gam2 <v, mu>, not on mu: the scalars agree, each mu is that of its own recurrence
    assert abs(l[5] - s[5]) <= 1e-6 * abs(s[5])
    assert 2 * l[3] <= s[3] and l[2] < s[2], (s[2:], l[2:])
    pc = pr.TwoGrid(A, 0, W, tau, gam2)
    assert pr.pcg(A, va, tau, gam2, 1, 500, pc)[1] == l[3]
    mu_b, steps_b, _ = pr.pcg(A, vb, tau, gam2, 0, 500, pc)
    assert steps_b == l[4] and np.linalg.norm(l[1] - mu_b) <= 1e-9 * np.linalg.norm(mu_b)


def test_reproducible_and_kind0_after_kind1_equals_never_enabled():
    N, M, W, tau, gam2 = 2000, 1024, 64, 2.0, 0.2
    bed, _ = _ld_problem(N, M)
    v = np.random.default_rng(6).standard_normal(M)

    def solve(sh):
        dv, dmu = sh.vecM(v), sh.vecM()
        st, _ = sh.cg_solve(dv, None, tau, gam2, 1, 300, dmu)
        return dmu.download(), st.iters

    with _shard(bed, N, M, W=W) as sh:
        x1, n1 = solve(sh)
        x2, n2 = solve(sh)
        assert np.array_equal(x1, x2) and n1 == n2
        sh.set_cg_precond("scalar", W)
        xs, ns = solve(sh)
    with _shard(bed, N, M, W=W) as sh:
        sh.set_cg_precond("scalar", W)
        x0, n0 = solve(sh)
    with capi.Shard(N, M, device=0) as sh:           # a context that never enabled it
        sh.set_layout(False, 2)
        sh.upload_bed(bed)
        sh.compute_markers_statistics()
        xn, nn = solve(sh)
    assert np.array_equal(xs, xn) and np.array_equal(x0, xn) and ns == nn == n0
    assert n1 < ns


def test_shard_windows_are_clipped_at_both_ends():
    N, M, W = 2000, 1000, 128
    bed, _ = _ld_problem(N, M)
    rows = np.array(bed, dtype=np.uint8).reshape(M, (N + 3) // 4)
    # a shard [S, S+M2) with S = 437: its first and last windows straddle the shard's ends and are clipped there
    S, M2, h = 437, 300, W // 2
    a, b, na, mave, msig = _host(rows[S:S + M2].ravel(), N, M2, S)
    with _shard(rows[S:S + M2].ravel(), N, M2, S=S, Mt=M, W=W) as sh:
        info = sh.precond_info()
        wins = pr.windows(S, M2, W)
        assert info["first_window"] == [min(k for g, k, _, _ in wins if g == 0), min(k for g, k, _, _ in wins if g == 1)]
        clipped = 0
        for grid, k, lo, hi in wins:
            wlo = k * W if grid == 0 else k * W - h
            assert lo == max(wlo, S) and hi == min(wlo + W, S + M2)
            clipped += (lo > wlo) + (hi < wlo + W)
            G = sh.precond_window_gram(grid, k)
            n = hi - lo
            ref = pr.gram_planes(a, b, na, mave, msig, S, lo, hi)
            assert np.max(np.abs(G[:n, :n] - ref)) <= 1e-12 * np.max(np.diag(ref)) and np.all(G[n:, :] == 0)
        assert clipped >= 2


def test_refusals():
    N, M = 600, 256
    bed = synth.synth_bed(N, M, seed=1, miss_ppm=5000)
    with capi.Shard(N, M, device=0) as sh:
        with pytest.raises(capi.GvError, match="window must be 32, 64 or 128"):
            sh.set_cg_precond("ld", 96)
        with pytest.raises(capi.GvError, match="kind must be"):
            sh.set_cg_precond(2, 128)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(bed)
        sh.set_kernel_mode(0)
        sh.compute_markers_statistics()
        sh.set_cg_precond("ld", 64)
        dv, dmu = sh.vecM(np.ones(M)), sh.vecM()
        with pytest.raises(capi.GvError, match="re-encoded"):
            sh.cg_solve(dv, None, 1.0, 1.0, 1, 10, dmu)
    with capi.Shard(N, M, device=0) as sh:        # the N-space solver
        sh.upload_bed(bed)
        sh.compute_markers_statistics()
        sh.compute_people_statistics()
        sh.set_cg_precond("ld", 64)
        vn, mn = sh.vecN(np.ones(4 * sh.mbytes)), sh.vecN()
        with pytest.raises(capi.GvError, match="refused while the LD preconditioner"):
            sh.cg_solve_aat(vn, None, 1.0, 1.0, 10, mn)
    with capi.Shard(N, M, device=0) as sh:        # dense (meth) data
        sh.synth_meth(3)
        with pytest.raises(capi.GvError, match="meth"):
            sh.set_cg_precond("ld", 64)
