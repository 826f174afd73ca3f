"""Restatement of the fixed-point route of 8-bit dosage codes (include/gvamp.h, gv_set_dosage_route), in Python
integers and numpy, kept apart from the library's code: quantisation, digits, the biased integer sums, the recombination.

    v -> q = rint(v 2^(54-e)),  2^(e-1) <= max|v| < 2^e           one exponent per vector
      -> 7 balanced base-256 digits d_l in [-128, 127]            q = sum_l d_l 256^l, exact
    ATx: S1[m] = sum_l 256^l sum_n (b_mn - 128) d_l[n]            the int32 column sums of the matrix pipe, recombined exactly
         Q     = sum_n q_n                                        one exact integer per pass
         out[m] = msig[m] scale (S1 - (mu'[m] - 128) Q) 2^(e-54) / sqrt(N)       each integer rounded once, one fma
    Ax : c = msig scale x in digits (exponent ec); e_m = (mu'_m - 128) c_m on the grid 2^7 coarser, qe = rint(e 2^(47-ec))
         T[n] = sum_l 256^l sum_m (b_mn - 128) dc_l[m],  E = sum_m qe_m
         out[n] = (T[n] - 128 E) 2^(ec-54) / sqrt(N)              the subtraction in integers, one rounding

The multiplier 2^(54-e) is at most 2^1000 (E_MIN); a vector with an entry that is not finite gives NaN everywhere.

The digit-plane sums are int64 matrix products (exact); everything above them is Python integers.  tests/test_dosage_fixed_cpu.py
replaces quantise, plane_sums, total, centre_weights and centre_term by subtly wrong ones to show what the GPU test would see."""
import math
from fractions import Fraction

import numpy as np

SEG_MAX = (2 ** 31 - 1) // (128 * 128)          # K-entries an int32 column sum can take: 131 071
INT32_MAX = 2 ** 31 - 1


SHIFT_MAX = 1000                                 # k_dm_quant: the multiplier 2^(54-e) stays representable -- at most 2^1000
E_MIN = 54 - SHIFT_MAX                           # so a vector with max|v| < 2^-946 is quantised as if its exponent were -946


def exponent(v):
    """e with 2^(e-1) <= max|v| < 2^e, but at least E_MIN (fewer bits below it, the same formulas); 0 for a zero vector -- every q is
    zero then, whatever e -- and None when an entry is not finite: every output of the product is NaN then"""
    v = np.asarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        return None
    amax = float(np.max(np.abs(v))) if len(v) else 0.0
    return max(math.frexp(amax)[1], E_MIN) if amax > 0 else 0


def quantise(v, e):
    """q = rint(v 2^(54-e)) as Python integers (the product by a power of two is exact), ties to even"""
    return [int(t) for t in np.rint(np.asarray(v, dtype=np.float64) * math.ldexp(1.0, 54 - e))]


def digits(q):
    """7 x len(q) int64: balanced base-256 digits in [-128, 127], q = sum_l d_l 256^l"""
    d = np.zeros((7, len(q)), dtype=np.int64)
    for k, t in enumerate(q):
        for l in range(7):
            dg = ((t + 128) % 256) - 128
            t = (t - dg) // 256
            d[l, k] = dg
        assert t == 0, "q does not fit 7 balanced digits"
    return d


def plane_sums(Bb, d):
    """the int32 sums of the matrix pipe, unsegmented: 7 x rows int64, plane l = Bb @ d_l with Bb = B - 128 (rows x K)"""
    return np.stack([Bb @ d[l] for l in range(7)])


def recombine(planes):
    """sum_l 256^l plane_l as Python integers"""
    return [sum(int(planes[l, r]) << (8 * l) for l in range(7)) for r in range(planes.shape[1])]


def fma(a, b, c):
    """a * b + c rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def code_mean(B, na=None):
    """mu' as the device holds it: the exact integer sum over the individuals with a phenotype, divided in float64"""
    B = np.asarray(B)
    nai = np.ones(B.shape[1], dtype=np.int64) if na is None else np.asarray(na).astype(np.int64)
    return (B.astype(np.int64) * nai[None, :]).sum(axis=1).astype(np.float64) / float(nai.sum())


def total(q):
    """the pass's one integer sum_k q_k (the limb sums of k_dm_quant, added in integers)"""
    return sum(q)


def centre_weights(mu, c, ec):
    """qe: e = (mu' - 128) c quantised on the grid 2^7 coarser than that of c"""
    return quantise((np.asarray(mu, dtype=np.float64) - 128.0) * c, ec + 7)


def centre_term(qe):
    """what the Ax epilogue subtracts from T[n], in units of the grid of c: 128 E"""
    return 128 * total(qe)


def atx(B, mu, msig, scale, p, planes_out=None):
    """route 1's ATx in float64: B M x N uint8, mu / msig float64 per marker, p the first N entries"""
    B = np.asarray(B)
    M, N = B.shape
    p = np.asarray(p, dtype=np.float64)[:N]
    e = exponent(p)
    if e is None:
        return np.full(M, np.nan)
    q = quantise(p, e)
    planes = plane_sums(B.astype(np.int64) - 128, digits(q))
    if planes_out is not None:
        planes_out.append(planes)
    S1, Q = recombine(planes), total(q)
    Qd, inv, isn = float(Q), math.ldexp(1.0, e - 54), 1.0 / math.sqrt(float(N))
    out = np.empty(M)
    for m in range(M):
        core = fma(-(float(mu[m]) - 128.0), Qd, float(S1[m]))
        out[m] = (float(msig[m]) * scale) * (core * inv) * isn
    return out


def ax(B, mu, msig, scale, x, planes_out=None):
    """route 1's Ax in float64 at the N individuals"""
    B = np.asarray(B)
    M, N = B.shape
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.asarray(msig, dtype=np.float64) * scale * np.asarray(x, dtype=np.float64)
    ec = exponent(c)
    if ec is None:
        return np.full(N, np.nan)
    qc = quantise(c, ec)
    qe = centre_weights(mu, c, ec)
    planes = plane_sums((B.astype(np.int64) - 128).T.copy(), digits(qc))
    if planes_out is not None:
        planes_out.append(planes)
    T, E128 = recombine(planes), centre_term(qe)
    inv, isn = math.ldexp(1.0, ec - 54), 1.0 / math.sqrt(float(N))
    return np.array([float(t - E128) * inv * isn for t in T])


def lmmse(B, mu, msig, scale, x, tau, gam2):
    """gv_lmmse_mult on route 1: z = Ax(x) (zeros at the pad slots, which ATx does not read), w = ATx(z), out = fma(tau, w, gam2 x) as the
    ATx epilogue k_dm_fin_atx forms it"""
    x = np.asarray(x, dtype=np.float64)
    w = atx(B, mu, msig, scale, ax(B, mu, msig, scale, x))
    return np.array([fma(tau, float(w[m]), gam2 * float(x[m])) for m in range(len(x))])


FLOOR = math.ldexp(1.0, E_MIN)      # the bounds are relative to the largest entry of the QUANTISED vector, but not below 2^E_MIN: under it
                                    # the per-entry error is 2^-55 2^E_MIN (SHIFT_MAX), not 2^-55 max|v|


def atx_bound(N, scale, msig, p):
    """the contract: N 2^-50 (255 scale / 2) msig[m] max|p| / sqrt(N), max|p| not below 2^E_MIN"""
    amax = max(float(np.max(np.abs(p))), FLOOR)
    return N * 2.0 ** -50 * (255.0 * scale / 2.0) * np.asarray(msig, dtype=np.float64) * amax / math.sqrt(N)


def ax_bound(N, M, scale, msig, x):
    """the contract: M 2^-50 (255 scale / 2) max|msig x| / sqrt(N), the weight scale max|msig x| not below 2^E_MIN"""
    amax = float(np.max(np.abs(np.asarray(msig, dtype=np.float64) * x)))
    if scale * amax < FLOOR:
        amax = FLOOR / scale
    return M * 2.0 ** -50 * (255.0 * scale / 2.0) * amax / math.sqrt(N)


# ---- inputs of the int32-bound tests: one digit plane is -128 at EVERY K-entry, so a row of code 0 (operand byte -128) gains +16 384
# per entry in that plane and a row of code 255 (operand byte +127) loses 16 256: past 131 071 entries an int32 sum would wrap.
BOUND_PLANE = 5


def bound_q(K, seed):
    """K integers |q| < 2^54, max in [2^53, 2^54), digit 5 == -128 everywhere; digit 6 varies in sign and size, digits 1..3 are random,
    digits 0 and 4 are zero (a change of q by a few units cannot carry into digit 5)"""
    rng = np.random.default_rng(seed)
    d6 = rng.integers(-60, 61, K)
    d6[0] = 60
    low = rng.integers(-2 ** 22, 2 ** 22, K) * 256
    return [int(a) * 2 ** 48 - 128 * 2 ** 40 + int(b) for a, b in zip(d6, low)]


def bound_atx_case():
    """(N, M) = (140 000, 70): B with row 3 all code 0 and row 5 all code 255 among synthetic rows; p = q 2^-54 (exact: q is even)"""
    from gvamp_amd import synth
    N, M = 140000, 70
    B = synth.synth_dosage(N, M, 77, 8)
    B[3], B[5] = 0, 255
    p = np.array([float(t) for t in bound_q(N, 1)]) * 2.0 ** -54
    return N, M, B, p


def bound_ax_rows(M):
    """which rows of the Ax bound matrix are ordinary (synthetic) and which are constant at 255; the rest are constant at 0"""
    m = np.arange(M)
    return m % 47 == 5, m % 470 == 7


def bound_ax_case():
    """(N, M) = (80, 140 000): most rows code 0, some code 255, every 47th synthetic; the target weights c = q 2^-54 -- the caller
    divides by msig scale to get x (constant rows have msig == 1)"""
    from gvamp_amd import synth
    N, M = 80, 140000
    ordinary, top = bound_ax_rows(M)
    B = np.zeros((M, N), dtype=np.uint8)
    B[ordinary] = synth.synth_dosage(N, int(ordinary.sum()), 78, 8)
    B[top] = 255
    c = np.array([float(t) for t in bound_q(M, 2)]) * 2.0 ** -54
    return N, M, B, c
