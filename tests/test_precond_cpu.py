"""The LD-block preconditioner's definitions on the CPU (tests/precond_restatement.py): the integer-plane Gram formula against the
dense A_w^T A_w, A against the oracle's Ax / ATx, and the step counts of two grids of windows against the scalar rule on LD data."""
import numpy as np
import pytest

from gvamp_amd import synth
import precond_restatement as pr


def _data(N, M, seed, ld_block=0, miss_ppm=5000, mask_every=0):
    bed = synth.synth_bed(N, M, seed=seed, miss_ppm=miss_ppm, ld_block=ld_block, ld_ppm=900000 if ld_block else 0)
    a, b = pr.decode(bed, N, M)
    na = np.ones(N)
    if mask_every:
        na[::mask_every] = 0.0
    mave, msig = pr.marker_stats(a, b, na)
    return bed, a, b, na, mave, msig


@pytest.mark.parametrize("N,mask_every,S,W", [(1001, 0, 0, 64), (1203, 7, 37, 128), (998, 3, 5, 32)])
def test_plane_formula_equals_dense_gram(N, mask_every, S, W):
    M = 300
    _, a, b, na, mave, msig = _data(N, M, seed=11, ld_block=48, miss_ppm=20000, mask_every=mask_every)
    A = pr.matrix(a, b, na, mave, msig)
    wins = pr.windows(S, M, W)
    assert {w[0] for w in wins} == {0, 1}
    for grid, k, lo, hi in wins:
        Gd = pr.gram_dense(A, S, lo, hi)
        Gp = pr.gram_planes(a, b, na, mave, msig, S, lo, hi)
        assert np.max(np.abs(Gd - Gp)) <= 1e-12 * np.max(np.diag(Gd)), (grid, k)


def test_windows_cover_every_marker_once_per_grid():
    S, M, W = 37, 300, 64
    for grid in (0, 1):
        cover = np.zeros(M, dtype=int)
        for g, k, lo, hi in pr.windows(S, M, W):
            if g == grid:
                assert lo >= S and hi <= S + M and hi > lo
                cover[lo - S:hi - S] += 1
        assert np.all(cover == 1)


def test_matrix_matches_oracle_products(oracle):
    N, M = 1001, 200
    bed, a, b, na, mave, msig = _data(N, M, seed=5, miss_ppm=30000)
    o_mave, o_msig = oracle.marker_stats(bed, N, M)
    assert np.allclose(mave, o_mave, rtol=1e-13, atol=1e-15) and np.allclose(msig, o_msig, rtol=1e-12)
    A = pr.matrix(a, b, na, mave, msig)
    x = np.random.default_rng(0).standard_normal(M)
    zf = oracle.ax(bed, N, M, o_mave, o_msig, x)
    z = zf[:N]
    assert np.linalg.norm(A @ x - z) <= 1e-12 * np.linalg.norm(z)
    w = oracle.atx(bed, N, M, o_mave, o_msig, zf)
    assert np.linalg.norm(A.T @ z - w) <= 1e-12 * np.linalg.norm(w)


@pytest.mark.parametrize("ld_block", [64, 48])
def test_two_grids_halve_the_cg_steps_on_ld_data(ld_block):
    N, M, W, tau = 3000, 2048, 128, 2.0
    _, a, b, na, mave, msig = _data(N, M, seed=77, ld_block=ld_block)
    A = pr.matrix(a, b, na, mave, msig)
    v = np.random.default_rng(1).standard_normal(M)
    for gam2 in (0.05, 0.5, 5.0):
        mu_s, n_s, ok_s = pr.pcg(A, v, tau, gam2, 1, 500)
        pc = pr.TwoGrid(A, 0, W, tau, gam2)
        mu_l, n_l, ok_l = pr.pcg(A, v, tau, gam2, 1, 500, pc)
        assert ok_s and ok_l and pc.fallback == 0
        assert np.linalg.norm(mu_l - mu_s) <= 2e-5 * np.linalg.norm(mu_s)
        if gam2 < 1:
            assert 2 * n_l <= n_s, (ld_block, gam2, n_s, n_l)
        else:
            assert n_l < n_s, (ld_block, gam2, n_s, n_l)


def test_driver_options_refuse_bad_values():
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gvamp_amd", "gvamp_sim")
    for args in (["--cg-precond", "block"], ["--cg-precond", "ld", "--cg-precond-window", "96"]):
        r = subprocess.run([exe] + args + ["--bed-file", "x"], capture_output=True, text=True)
        assert r.returncode != 0 and "FATAL" in r.stdout and "--cg-precond" in r.stdout, (args, r.stdout[-500:])
