"""The yardstick of tests/test_gpu_assoc.py checked on the CPU: the long-double restatement of the association test against the
oracle's p-values and against scipy's linear regression, and the declarations of include/gvamp.h."""
import os
import re

import numpy as np
import pytest

import assoc_restatement as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_restatement_p_equals_the_oracle_loo_and_loco(oracle):
    """missing genotypes, 2 % NA phenotypes, an empty chromosome (the case of test_gpu_pvals.py): the project's p-value bar"""
    from gvamp_amd import synth
    N, M = 1203, 900
    rng = np.random.default_rng(21)
    bed = synth.synth_bed(N, M, seed=55, miss_ppm=15000)
    present = rng.random(N) >= 0.02
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(present)[0]:
        m4[n >> 2] |= 1 << (n & 3)
    nonas = int(present.sum())
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.05) * 3.0
    chrom = np.sort(rng.integers(1, 24, M)).astype(np.int32)
    chrom[chrom == 7] = 8
    mave, msig = oracle.marker_stats(bed, N, M, mask4=m4, nonas=nonas)
    z1 = oracle.ax(bed, N, M, mave, msig, x1, mask4=m4)
    y = np.zeros(4 * ((N + 3) // 4))
    y[:N] = (z1[:N] + rng.standard_normal(N)) * present
    G, have = ar.decode_bed(bed, N, M)
    assert not have.all()
    V, b = ar.bed_columns(G, have, mave, msig)
    for ch in (None, chrom):
        want = oracle.pvals(bed, N, M, z1, y, x1, chrom=ch, mask4=m4, nonas=nonas, nthreads=4)
        got = ar.assoc(V, b, present, y, z1, x1, chrom=ch)
        assert want.min() < 1e-3
        assert np.allclose(got["p"].astype(np.float64), want, rtol=1e-8, atol=0)
        ok = np.isfinite(got["t"]) & (got["t"] != 0)
        assert np.all(np.sign(got["t"][ok]) == np.sign(got["beta"][ok])) and np.all(got["se"][ok] > 0)
        # se is beta / t written another way
        assert np.allclose((got["beta"][ok] / got["t"][ok]).astype(np.float64), got["se"][ok].astype(np.float64), rtol=1e-12, atol=0)


def test_restatement_equals_scipy_linregress_without_missing_data():
    """beta, se, t, p of the restatement are those of an ordinary regression of the residual on the standardised column"""
    stats = pytest.importorskip("scipy.stats")
    from gvamp_amd import synth
    N, M = 301, 40
    rng = np.random.default_rng(5)
    codes = synth.synth_dosage(N, M, 12, 8)
    na = np.ones(N)
    V, b, _msig = ar.dosage_columns(codes, 1.0 / 127.0, na)
    x1 = np.zeros(M)
    x1[[3, 17, 30]] = np.sqrt(N) * np.array([0.6, -0.4, 0.1])
    z1 = ((V.T @ x1.astype(LD)) / np.sqrt(LD(N))).astype(np.float64)
    y = z1 + rng.standard_normal(N)
    got = ar.assoc(V, b, na, y, z1, x1)
    assert got["p"].min() < 1e-10 and (got["t"] > 0).any() and (got["t"] < 0).any()
    for k in range(M):
        col = V[k].astype(np.float64)
        resid = y - z1 + col * x1[k] / np.sqrt(N)             # leave-one-out: the marker's own effect back in
        r = stats.linregress(col, resid)
        assert np.isclose(float(got["beta"][k]), r.slope, rtol=1e-9, atol=0)
        assert np.isclose(float(got["se"][k]), r.stderr, rtol=1e-9, atol=0)
        assert np.isclose(float(got["t"][k]), r.slope / r.stderr, rtol=1e-9, atol=0)
        assert np.isclose(float(got["p"][k]), r.pvalue, rtol=1e-8, atol=0)


def test_student_t_tail_of_the_restatement_at_known_values():
    """closed forms: nu = 1 (Cauchy) p = 1 - 2 atan(t) / pi; nu = 2: p = 1 - t / sqrt(2 + t^2)"""
    t = np.array([0.0, 1e-3, 0.5, 1.0, 3.0, 40.0])
    assert np.allclose(ar.t_two_sided(t, 1.0).astype(np.float64), 1 - 2 * np.arctan(t) / np.pi, rtol=1e-13, atol=0)
    assert np.allclose(ar.t_two_sided(t, 2.0).astype(np.float64), 1 - t / np.sqrt(2 + t * t), rtol=1e-12, atol=0)
    assert np.isnan(ar.t_two_sided(np.array([np.nan]), 5.0))[0]


def test_fewer_than_three_observations_give_nan_in_every_output():
    """two points always lie on a line: beta would be finite, 1 - rxy^2 is 0 or a rounding error of either sign, and se, t come out as
    NaN, inf or 0 by the last bit of it.  include/gvamp.h: n < 3 gives NaN in all four outputs"""
    x, y = np.array([0.5, -1.5], dtype=LD), np.array([0.3, 0.9], dtype=LD)
    for n in (0, 1, 2):
        r = ar.reg1d(x[:n].sum(keepdims=True), (x[:n] ** 2).sum(keepdims=True), (x[:n] * y[:n]).sum(keepdims=True),
                     y[:n].sum(keepdims=True), (y[:n] ** 2).sum(keepdims=True), np.array([n], dtype=LD))
        assert all(np.isnan(r[k][0]) for k in ("beta", "se", "t", "p")), (n, r)
    x, y = np.array([0.5, -1.5, 1.0], dtype=LD), np.array([0.3, 0.9, -0.2], dtype=LD)
    r = ar.reg1d(x.sum(keepdims=True), (x ** 2).sum(keepdims=True), (x * y).sum(keepdims=True), y.sum(keepdims=True),
                 (y ** 2).sum(keepdims=True), np.array([3], dtype=LD))
    assert all(np.isfinite(r[k][0]) for k in ("beta", "se", "t", "p")) and 0 < r["p"][0] < 1


def test_header_declares_the_assoc_family_and_the_abi_version_stays():
    txt = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    assert re.search(r"^#define GV_ABI_VERSION 4$", txt, flags=re.M)
    assert re.search(r"typedef struct \{ double \*beta, \*se, \*t, \*p; \} gv_assoc_out;", txt)
    assert re.search(r"^int gv_assoc_loo\(gv_ctx\* ctx, const gv_vec\* z1, const gv_vec\* y, const gv_vec\* x1_hat, const gv_assoc_out\* out\);",
                     txt, flags=re.M)
    assert re.search(r"^int gv_assoc_loco\(gv_ctx\* ctx, const gv_vec\* z1, const gv_vec\* y, const gv_vec\* x1_hat, const int\* chrom,\s*"
                     r"const gv_assoc_out\* out, double\* chrom_pred\);", txt, flags=re.M)
    # the refusal lists of gv_pvals_* stay word for word
    assert "gv_pvals_* (its meth branch of pvals_calc, data.cpp:1187-1223, computes and stores nothing);" in txt
    assert "gv_download_bed, gv_people_stats, gv_cg_solve_aat*, gv_pvals_*, gv_set_decomp -- and gv_set_cg_precond kind 1." in txt
    from gvamp_amd import capi
    assert "gv_assoc_loo" in capi.EXPORTS and "gv_assoc_loco" in capi.EXPORTS
