"""The LD-block preconditioner of 8-bit dosage codes, the parts that need no GPU: the integer Gram of
tests/precond_dosage_restatement.py against the dense A^T A block of the decoded matrix in long double, the step counts of two grids of
windows against the scalar rule on gv_synth_dosage_ld's codes, the host twin of that synthesiser, and the new C-ABI names."""
import os
import re
import subprocess

import numpy as np
import pytest

import ld_dosage_restatement as ldd
import precond_dosage_restatement as pdr
import precond_restatement as pr
from gvamp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW_NAMES = ("gv_synth_dosage_ld",)
PINNED = "gv_download_bed, gv_people_stats, gv_cg_solve_aat*, gv_pvals_*, gv_set_decomp -- and gv_set_cg_precond kind 1."


def _codes(case, N=1003, M=300):
    """(codes, na, missing) of the four cases the Gram is held on"""
    if case == "rare":
        return ldd.rare_rows(), None, False
    codes = synth.synth_dosage_ld(N, M, 11, 8, 48, 900000, miss_ppm=20000 if case == "missing" else 0)
    na = None
    if case == "masked":
        na = np.ones(N)
        na[::7] = 0.0
    return codes, na, case == "missing"


@pytest.mark.parametrize("case,S,W", [("complete", 0, 64), ("masked", 37, 128), ("missing", 5, 32), ("rare", 37, 128)])
def test_integer_gram_equals_the_dense_block_in_long_double(case, S, W):
    codes, na, missing = _codes(case)
    M = codes.shape[0]
    assert bool(np.any(codes == 255)) == missing
    A = pdr.matrix(codes, na, missing)                       # long double
    wins = pr.windows(S, M, W)
    assert {w[0] for w in wins} == {0, 1}
    worst = 0.0
    for grid, k, lo, hi in wins:
        Aw = A[:, lo - S:hi - S]
        Gd = Aw.T @ Aw
        G = pdr.window_gram(codes, S, lo, hi, na, missing)
        assert G.dtype == np.float64 and np.array_equal(G, G.T), (grid, k)          # G_jk and G_kj are the same bits
        err = float(np.max(np.abs(G.astype(LD) - Gd)) / np.max(np.diag(Gd)))
        worst = max(worst, err)
        assert err <= 1e-12, (case, grid, k, err)
    print("%s: max |G - dense| / max diag = %.3e" % (case, worst))


def test_rows_without_a_present_individual_and_constant_rows_give_exact_zeros():
    N = 77
    codes = np.random.default_rng(1).integers(0, 255, size=(5, N), dtype=np.uint8)
    codes[1] = 253                      # constant: X_jj = 0 exactly
    codes[2] = 255                      # all missing: c_j = 0
    na = np.ones(N)
    na[::5] = 0.0
    codes[3, na != 0] = 255             # present only at masked individuals: c_j = 0 too
    G = pdr.gram(codes, na, missing=True)
    assert G[1, 1] == 0.0 and np.all(G[2] == 0.0) and np.all(G[:, 2] == 0.0) and np.all(G[3] == 0.0) and np.all(G[:, 3] == 0.0)
    assert G[0, 0] > 0 and G[4, 4] > 0 and np.all(np.isfinite(G))


@pytest.mark.parametrize("miss_ppm", [0, 20000])
@pytest.mark.parametrize("ld_block", [64, 48])
def test_two_grids_halve_the_cg_steps_on_ld_dosage_codes(ld_block, miss_ppm):
    """the pilot's table: N = 3000 x M = 2048, seed 77, tau = 2, W = 128"""
    N, M, W, tau = 3000, 2048, 128, 2.0
    codes = synth.synth_dosage_ld(N, M, 77, 8, ld_block, 900000, miss_ppm=miss_ppm)
    A = np.asarray(pdr.matrix(codes, None, miss_ppm > 0, dtype=np.float64))
    v = np.random.default_rng(1).standard_normal(M)
    for gam2 in (0.05, 0.5, 5.0):
        mu_s, n_s, ok_s = pr.pcg(A, v, tau, gam2, 1, 500)
        pc = pr.TwoGrid(A, 0, W, tau, gam2)
        mu_l, n_l, ok_l = pr.pcg(A, v, tau, gam2, 1, 500, pc)
        print("ld_block %d miss_ppm %d gam2 %g: %d -> %d steps, mu rel %.2e" %
              (ld_block, miss_ppm, gam2, n_s, n_l, np.linalg.norm(mu_l - mu_s) / np.linalg.norm(mu_s)))
        assert ok_s and ok_l and pc.fallback == 0
        assert np.linalg.norm(mu_l - mu_s) <= 2e-5 * np.linalg.norm(mu_s)
        if gam2 < 1:
            assert 2 * n_l <= n_s, (ld_block, miss_ppm, gam2, n_s, n_l)
        else:
            assert n_l < n_s, (ld_block, miss_ppm, gam2, n_s, n_l)


def test_synth_dosage_ld_recipe():
    N, M = 403, 70
    for bits in (8, 16):
        res = (1 << bits) - 1
        a = synth.synth_dosage_ld(N, M, 1234, bits, 16, 900000)
        assert a.shape == (M, N) and a.dtype == (np.uint8 if bits == 8 else np.uint16) and not np.any(a == res)
        assert np.array_equal(a, synth.synth_dosage_ld(N, M, 1234, bits, 16, 900000))
        assert np.array_equal(synth.synth_dosage_ld(N, M, 1234, bits, 16, 900000, S=0)[6:], synth.synth_dosage_ld(N, M - 6, 1234, bits, 16, 900000, S=6))
        # no LD draw and no missing draw: synth_dosage's codes clamped one below the reserved one
        assert np.array_equal(synth.synth_dosage_ld(N, M, 1234, bits, 16, 0), synth.synth_dosage_na(N, M, 1234, bits, 0))
        # the missing draw is a hash of its own: it changes nothing else, and it differs from synth_dosage_na's
        m = synth.synth_dosage_ld(N, M, 1234, bits, 16, 900000, miss_ppm=20000)
        miss = m == res
        assert 0.01 < miss.mean() < 0.03 and np.array_equal(m[~miss], a[~miss])
        assert not np.array_equal(miss, synth.synth_dosage_na(N, M, 1234, bits, 20000) == res)
    with pytest.raises(ValueError):
        synth.synth_dosage_ld(N, M, 1, 12, 16, 900000)
    with pytest.raises(ValueError):
        synth.synth_dosage_ld(N, M, 1, 8, 0, 900000)


@pytest.mark.parametrize("ld_block,want", [(64, 16.0), (48, 12.8)])
def test_synth_dosage_ld_gives_the_ld_the_pilot_states(ld_block, want):
    """mean sum of r^2 over 48 markers on each side at N = 3000 x M = 2048, seed 77, ld_ppm 900000 (the issue's figures, to 0.1)"""
    codes = synth.synth_dosage_ld(3000, 2048, 77, 8, ld_block, 900000)
    r2 = np.corrcoef(codes.astype(np.float64)) ** 2
    j = np.arange(2048)
    band = np.abs(j[:, None] - j[None, :]) <= 48
    got = float(np.where(band, r2, 0.0).sum(1).mean())
    print("ld_block %d: mean sum r^2 = %.2f" % (ld_block, got))
    assert abs(got - want) < 0.1


def test_new_names_are_declared_and_bound_and_the_pinned_sentence_stays():
    hdr = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    for n in NEW_NAMES:
        assert re.search(r"\bint %s\(" % n, hdr), n
        assert n in capi.EXPORTS, n
    assert re.search(r"#define GV_ABI_VERSION 4\b", hdr)
    assert hasattr(capi.Shard, "synth_dosage_ld") and hasattr(synth, "synth_dosage_ld")
    assert PINNED in hdr
    after = hdr[hdr.index(PINNED) + len(PINNED):][:400]
    assert "gv_set_ld_dosage(ctx, 1)" in after and "exception" in after          # the exception is stated right after it
    assert "((s_j * s_k) * (1 / N)) * (fl(X_jk) / (fl(c_j) * fl(c_k)))" in hdr     # the one evaluation order


def test_options_refuse_nothing_new():
    """--ld-dosage 1 beside --cg-precond ld parses for every --geno-format: the run gets as far as its --run-mode"""
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    for fmt in ("bed", "dosage8", "dosage16"):
        r = subprocess.run([exe, "--run-mode", "nonsense", "--bed-file", "x", "--geno-format", fmt, "--ld-dosage", "1", "--cg-precond", "ld",
                            "--cg-precond-window", "64"], capture_output=True, text=True)
        assert r.returncode != 0 and "unknown --run-mode" in r.stdout, (fmt, r.stdout[-500:])
