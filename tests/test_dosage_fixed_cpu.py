"""The fixed-point route of 8-bit dosage codes (gv_set_dosage_route), the parts that need no GPU: its restatement in integers
(tests/dosage_fixed_restatement.py) held to the long-double restatement of the dosage kind (tests/test_gpu_dosage.py), the inputs of
the int32-bound tests, and the new C-ABI names."""
import os
import re
import subprocess

import numpy as np
import pytest

import dosage_fixed_restatement as fx
import test_gpu_dosage as gd
from gvamp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW_NAMES = ("gv_set_dosage_route", "gv_get_dosage_route")


@pytest.mark.parametrize("scale", [1.0 / 127.0, 1.0 / 64.0])
@pytest.mark.parametrize("N,M", [(5, 3), (1003, 700), (257, 7001)])
def test_restatement_meets_the_contract_and_the_bar_of_the_dosage_products(N, M, scale):
    B = gd.codes_matrix(N, M, 8, N * 7 + M)
    m4, na, nonas = gd.na_mask(N, True)
    rng = np.random.default_rng(N + M)
    x, p = rng.standard_normal(M), rng.standard_normal(N)
    mu, q, D = gd.ref_code_stats(B, na, nonas)
    _, rs = gd.ref_stats(mu, q, nonas, scale, 1.0)
    msig, mu64 = rs.astype(np.float64), fx.code_mean(B, na)
    assert np.allclose(mu64, mu.astype(np.float64), rtol=1e-15, atol=0)
    rw = gd.ref_atx(D @ p.astype(LD), rs, scale, N)
    rz = gd.ref_ax(D, rs, scale, x, N)
    w, z = fx.atx(B, mu64, msig, scale, p), fx.ax(B, mu64, msig, scale, x)
    ew, ez = np.abs(w.astype(LD) - rw), np.abs(z.astype(LD) - rz)
    bw, bz = fx.atx_bound(N, scale, msig, p), fx.ax_bound(N, M, scale, msig, x)
    print("ATx rel %.3e  worst error / bound %.3e;  Ax rel %.3e  worst error / bound %.3e"
          % (gd.rel(w, rw), float(np.max(ew / bw)), gd.rel(z, rz), float(np.max(ez)) / bz))
    assert np.all(ew <= bw) and np.all(ez <= bz)
    assert gd.rel(w, rw) < 1e-13 and gd.rel(z, rz) < 1e-13


def test_digits_are_balanced_and_exact():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(500) * 10.0 ** rng.uniform(-9, 3, 500)
    e = fx.exponent(v)
    assert 2.0 ** (e - 1) <= np.max(np.abs(v)) < 2.0 ** e
    q = fx.quantise(v, e)
    assert max(abs(t) for t in q) <= 2 ** 54
    d = fx.digits(q)
    assert d.min() >= -128 and d.max() <= 127
    assert [sum(int(d[l, k]) << (8 * l) for l in range(7)) for k in range(len(q))] == q
    assert np.all(np.abs(np.array(q, dtype=LD) * LD(2.0) ** (e - 54) - v.astype(LD)) <= LD(2.0) ** (e - 55))


def test_the_bound_inputs_overflow_an_unsegmented_int32_sum():
    """what the GPU tests of the int32 bound rest on: with these inputs a column sum of one digit plane over ALL K-entries exceeds
    2^31 - 1 in magnitude, so a kernel that did not flush its int32 accumulators could not give the right answer"""
    assert fx.SEG_MAX == 131071 and fx.SEG_MAX * 16384 <= fx.INT32_MAX < (fx.SEG_MAX + 1) * 16384
    # ATx: K = individuals
    N, M, B, p = fx.bound_atx_case()
    assert N > fx.SEG_MAX and np.all(B[3] == 0) and np.all(B[5] == 255) and np.all(B[4].min() != B[4].max())
    e = fx.exponent(p)
    d = fx.digits(fx.quantise(p, e))
    assert e == 0 and np.all(d[fx.BOUND_PLANE] == -128)
    assert d[6].min() < -30 and d[6].max() > 30                      # the vector itself varies in sign and size
    col = (B.astype(np.int64) - 128) @ d[fx.BOUND_PLANE]
    print("ATx plane %d sums: row of code 0 %d, row of code 255 %d" % (fx.BOUND_PLANE, col[3], col[5]))
    assert col[3] > fx.INT32_MAX and col[5] < -fx.INT32_MAX - 1
    # Ax: K = markers; the weights are c = msig scale x, constant rows have msig == 1, a perturbation of c by a few ulps (msig of the
    # ordinary rows as the device rounds it) cannot reach the plane
    N, M, B, c = fx.bound_ax_case()
    ordinary, top = fx.bound_ax_rows(M)
    assert M > fx.SEG_MAX and ordinary.sum() > 2000 and top.sum() > 200
    ec = fx.exponent(c)
    for cc in (c, c * (1 + 2.0 ** -50), c * (1 - 2.0 ** -50)):
        d = fx.digits(fx.quantise(cc, ec))
        assert ec == 0 and np.all(d[fx.BOUND_PLANE] == -128)
    col = (B.astype(np.int64) - 128).T @ d[fx.BOUND_PLANE]
    print("Ax plane %d sums over the markers: min %d max %d" % (fx.BOUND_PLANE, col.min(), col.max()))
    assert col.min() > fx.INT32_MAX


def test_new_abi_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gvamp.h")) as f:
        hdr = f.read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+GV_ABI_VERSION\s+4\b", hdr)          # additions only
    lib = os.path.join(ROOT, "gvamp_amd", "libgvamp.so")
    assert os.path.exists(lib), "libgvamp.so is built by build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_gvamp_main_real_checks_dosage_kernels_before_device_work():
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    assert os.path.exists(exe), "gvamp_main_real is built by build() (gvamp_amd/csrc/host/Makefile)"
    for a in ("fast", "1", ""):
        r = subprocess.run([exe, "--dosage-kernels", a], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--dosage-kernels" in r.stdout + r.stderr
