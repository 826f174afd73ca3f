"""The fixed-point route of 8-bit dosage codes (gv_set_dosage_route), the parts that need no GPU: its restatement in integers
(tests/dosage_fixed_restatement.py) held to the long-double restatement of the dosage kind (tests/test_gpu_dosage.py) and, at the
special vectors, to the exact rational product; the inputs of the int32-bound tests; the inputs of the bit-for-bit GPU test
(tests/dosage_fixed_cases.py): which digit edges they reach, and that a subtly wrong restatement changes output bits on them; and
the new C-ABI names."""
import decimal
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dosage_fixed_cases as dc
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


# ---- the inputs of tests/test_gpu_dosage_fixed.py ------------------------------------------------------------------------------------
def _drop_plane_0(Bb, d):
    d = d.copy()
    d[0] = 0
    return np.stack([Bb @ d[l] for l in range(7)])


def _trunc(v, e):
    return [int(t) for t in np.trunc(np.asarray(v, dtype=np.float64) * math.ldexp(1.0, 54 - e))]


def _half_away(v, e):
    s = np.asarray(v, dtype=np.float64) * math.ldexp(1.0, 54 - e)
    r, t = np.rint(s), np.trunc(s)
    tie = np.abs(s - t) == 0.5
    r[tie] = t[tie] + np.sign(s[tie])
    return [int(a) for a in r]


def _sum_of_doubles(q):
    acc = 0.0
    for t in q:
        acc += float(t)
    return int(acc)


# name -> (what replaces which stage of the restatement, the products it can touch, the vectors it is asked of)
MUTANTS = {
    "plane 0 dropped": (dict(plane_sums=_drop_plane_0), ("ATx", "Ax"), dc.KINDS),
    "truncating quantiser": (dict(quantise=_trunc), ("ATx", "Ax"), dc.KINDS),
    "round-half-away quantiser": (dict(quantise=_half_away), ("ATx", "Ax"), ("edge-pow2", "edge-top")),
    "Q / E from a sum of doubles": (dict(total=_sum_of_doubles), ("ATx", "Ax"), dc.KINDS),
    "qe on the grid of qc": (dict(centre_weights=lambda mu, c, ec: fx.quantise((np.asarray(mu) - 128.0) * c, ec),
                                  centre_term=lambda qe: fx.total(qe)), ("Ax",), dc.KINDS),
    "bias 127 in the E term": (dict(centre_weights=lambda mu, c, ec: fx.quantise((np.asarray(mu) - 127.0) * c, ec + 7)), ("Ax",),
                               dc.KINDS),
}
SENSITIVE_SHAPES = [s for s in dc.SHAPES if s[0] >= dc.SENSITIVE and s[1] >= dc.SENSITIVE]


@pytest.mark.parametrize("N,M,with_na", SENSITIVE_SHAPES)
def test_every_mutant_of_the_restatement_changes_bits_on_the_inputs_of_the_gpu_test(N, M, with_na, monkeypatch):
    """the strength of tests/test_gpu_dosage_fixed.py as a property of its inputs: each mutant below -- a kernel that is wrong in the
    lowest digit plane, in the rounding mode, in the integer sums, in the grid or the bias of the centring term -- changes at least one
    entry of each product it can touch, on EVERY vector it is asked of (the shares are printed).  One exception: a sum of doubles may
    land on the correctly rounded integer sum by the luck of its order (it does for single vectors at 200 x 513 and 513 x 128), so of
    that mutant at least one vector per shape and product must tell.  Shapes under 63 are exempt: at 5 x 3 a truncating quantiser
    changes no Ax entry"""
    cs = dc.case(N, M, with_na)
    msig = dc.host_msig(cs)
    B, mu = cs["B"], cs["mu"]
    vec = {k: (dc.x_vector(k, cs, msig), dc.p_vector(k, cs)) for k in dc.KINDS}
    base = {k: dict(Ax=fx.ax(B, mu, msig, dc.SCALE, x), ATx=fx.atx(B, mu, msig, dc.SCALE, p)) for k, (x, p) in vec.items()}
    for name, (patch, products, kinds) in MUTANTS.items():
        told = dict.fromkeys(products, 0)
        with monkeypatch.context() as mp:
            for attr, fn in patch.items():
                mp.setattr(fx, attr, fn)
            for k in kinds:
                x, p = vec[k]
                out = dict(Ax=fx.ax(B, mu, msig, dc.SCALE, x)) if products == ("Ax",) else \
                    dict(Ax=fx.ax(B, mu, msig, dc.SCALE, x), ATx=fx.atx(B, mu, msig, dc.SCALE, p))
                share = {pr: float(np.mean(out[pr] != base[k][pr])) for pr in products}
                print("%-28s %-10s %s" % (name, k, "  ".join("%s %5.1f %%" % (pr, 100 * share[pr]) for pr in products)))
                for pr in products:
                    told[pr] += share[pr] > 0
                    assert share[pr] > 0 or "sum of doubles" in name, (name, k, pr)
        assert all(told.values()), (name, told)


@pytest.mark.parametrize("N,M,with_na", dc.SHAPES)
def test_the_edge_vectors_reach_the_digit_edges(N, M, with_na):
    """digits -128 and +127 in the planes 0..5 (|q| <= 2^54 keeps plane 6 within +-64), a carry through all seven digits, ties that
    round-half-away would send elsewhere, the largest |q| a double allows (2^54 - 2: 2^54 itself is out of reach, v < 2^e has 53 bits)
    and a maximum that is a power of two; fx.digits asserts that every q fits.  On the Ax side for the weights c = msig scale x"""
    cs = dc.case(N, M, with_na)
    msig = dc.host_msig(cs)
    for kind, top in (("edge-pow2", False), ("edge-top", True)):
        rp = dc.edge_report(dc.p_vector(kind, cs))
        rc = dc.edge_report(dc.weights(msig, dc.x_vector(kind, cs, msig)))
        assert rp["e"] == -25 and (rc["e"] == -30 or M < dc.SENSITIVE)
        if N >= dc.SENSITIVE:
            dc.assert_edges(rp, top)
        if M >= dc.SENSITIVE:
            dc.assert_edges(rc, top)
    # the exponents of the two slots of a two-vector call are 20 apart and more
    assert abs(fx.exponent(dc.p_vector("normal", cs)) - (-25)) >= 20
    assert abs(fx.exponent(dc.weights(msig, dc.x_vector("normal", cs, msig))) - (-30)) >= 20 or M < dc.SENSITIVE


@pytest.mark.parametrize("N,M,with_na", SENSITIVE_SHAPES)
def test_the_ax_inputs_take_the_negative_low_limb_path_of_the_carry(N, M, with_na):
    """k_dm_fin_ax hands limbs_to_double the low limb tl - 128 el before the carry: tl = the planes 0..3 of T[n], el = the sum of the
    low 32 bits of qe, which are not negative -- so the limb is negative wherever qe is not zero throughout, and the inputs must reach
    that path (they do in every entry; the zero vector of the GPU test takes the other one): a wrong carry would then show"""
    cs = dc.case(N, M, with_na)
    msig = dc.host_msig(cs)
    neg = pos = 0
    for k in dc.KINDS:
        x = dc.x_vector(k, cs, msig)
        c = dc.weights(msig, x)
        planes = []
        fx.ax(cs["B"], cs["mu"], msig, dc.SCALE, x, planes_out=planes)
        el = sum(t & 0xFFFFFFFF for t in fx.centre_weights(cs["mu"], c, fx.exponent(c)))
        lo = [sum(int(planes[0][l, n]) << (8 * l) for l in range(4)) - 128 * el for n in range(N)]
        neg += sum(t < 0 for t in lo)
        pos += sum(t >= 0 for t in lo)
        assert mu_off_centre(cs["mu"])
    print("low limb of T - 128 E: negative at %d entries, non-negative at %d" % (neg, pos))
    assert neg > 0


def mu_off_centre(mu):
    return np.mean(mu != 128.0) > 0.9


def _exact(cs, msig, x, p):
    """the products of the definition in rationals, TIMES sqrt(N): mu' = (sum of the present codes) / nonas exactly"""
    B, na = cs["B"].astype(object), cs["na"].astype(np.int64)
    mu = [Fraction(int((cs["B"][m].astype(np.int64) * na).sum()), cs["nonas"]) for m in range(cs["M"])]
    w = [Fraction(float(msig[m])) * Fraction(dc.SCALE) for m in range(cs["M"])]
    fp, fxv = [Fraction(float(t)) for t in p], [Fraction(float(t)) for t in x]
    atx = [w[m] * sum((int(B[m, n]) - mu[m]) * fp[n] for n in range(cs["N"])) for m in range(cs["M"])]
    ax = [sum((int(B[m, n]) - mu[m]) * w[m] * fxv[m] for m in range(cs["M"])) for n in range(cs["N"])]
    return ax, atx


@pytest.mark.parametrize("kind", dc.SPECIAL)
@pytest.mark.parametrize("N,M,with_na", [(63, 17, False), (130, 70, True)])
def test_restatement_at_the_special_vectors_meets_the_contract(N, M, with_na, kind):
    """the zero vector gives zeros, a vector with an entry that is not finite NaN everywhere; under the cap of the multiplier
    (max|v| < 2^-946: q = rint(v 2^1000)) and beside subnormal entries the error against the exact rational product stays within the
    contract, whose max|v| does not go below 2^-946"""
    cs = dc.case(N, M, with_na)
    msig = dc.host_msig(cs)
    x, p = dc.x_vector(kind, cs, msig), dc.p_vector(kind, cs)
    z, w = fx.ax(cs["B"], cs["mu"], msig, dc.SCALE, x), fx.atx(cs["B"], cs["mu"], msig, dc.SCALE, p)
    assert z.shape == (N,) and w.shape == (M,)
    if kind == "zero":
        assert not z.any() and not w.any()
        return
    if kind in ("nan", "inf"):
        assert fx.exponent(p) is None and np.all(np.isnan(z)) and np.all(np.isnan(w))
        return
    if kind == "tiny":
        assert fx.exponent(p) == fx.E_MIN == -946 and np.max(np.abs(p)) < 2.0 ** -950 and np.any(np.abs(p) < 2.0 ** -1022)
        assert fx.exponent(dc.weights(msig, x)) == fx.E_MIN
    else:
        assert np.any((p != 0) & (np.abs(p) < 2.0 ** -1022)) and fx.exponent(p) > 0
    assert np.any(z != 0) and np.any(w != 0)
    rz, rw = _exact(cs, msig, x, p)
    sq = Fraction(decimal.Context(prec=60).sqrt(decimal.Decimal(N)))
    bz, bw = fx.ax_bound(N, M, dc.SCALE, msig, x), fx.atx_bound(N, dc.SCALE, msig, p)
    ez = max(abs(Fraction(float(z[n])) - rz[n] / sq) for n in range(N))
    ew = max(abs(Fraction(float(w[m])) - rw[m] / sq) / Fraction(float(bw[m])) for m in range(M))
    print("%s: Ax worst error / bound %.3e  ATx worst error / bound %.3e" % (kind, float(ez / Fraction(bz)), float(ew)))
    assert ez <= Fraction(bz) and ew <= 1


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
