"""Inputs of the bit-for-bit tests of the fixed-point route of 8-bit dosage codes (tests/test_gpu_dosage_fixed.py), built without a
GPU so that tests/test_dosage_fixed_cpu.py can show on the very same inputs that a subtly wrong kernel would change output bits.

Shapes: the smallest that reach each structural edge of k_dm_atx / k_dm_ax.  Vectors: ordinary ones, a wide dynamic range, and digit
edges built from integers q and passed as q 2^(e-54) -- on the Ax side the quantised vector is c = msig scale x, so x is solved for
from the weights wanted (x_edge)."""
import functools
import math

import numpy as np

import dosage_fixed_restatement as fx
import test_gpu_dosage as gd

SCALE = 1.0 / 127.0
TAU, GAM2 = 1.7, 0.35

# (N, M, phenotype mask).  Row pitch = N rounded up to 64; k_dm_atx steps 128 individuals, k_dm_ax 64 markers; a workgroup is 4 waves
# of 128 rows (ATx) / 128 individuals (Ax).
SHAPES = [
    (1, 1, False),            # less than one tile
    (5, 3, False),            # less than one tile, more than one row
    (63, 17, False),          # under one K-step on both sides
    (130, 70, False),         # pitch 192 = 3 x 64: the second half of the last ATx step is re-read from the first (k1 = k0); the last
                              # Ax column block is half outside the pitch (col >= pitch)
    (200, 513, False),        # pitch 256 = 4 x 64, the contrast; M = 513: five 128-row blocks -- a second k_dm_atx workgroup with idle
                              # waves, the m >= M row clamp -- and a last Ax step of one marker
    (513, 128, False),        # N = 513: five column blocks, a second k_dm_ax workgroup with idle waves; pitch 576 = 9 x 64; M = 128: no
                              # partial Ax step (the k0 + 64 <= M branch only)
    (1003, 700, False),       # several steps and segments on both sides
    (1003, 700, True),        # mu' over the individuals with a phenotype, the sums over all of them
    (4099, 3001, False),      # a larger mixed case: 33 ATx steps, 47 Ax steps, pitch 4160 = 65 x 64
]
# GV_DOSAGE_MFMA_SEG: the library's own cut, one K-step per segment (gather adds many pieces), and a length between the two (at the
# shapes of one or two K-steps there is nothing between: it coincides with one of the others there)
SEGS = (None, 256, 64)
KINDS = ("normal", "decades", "edge-pow2", "edge-top")
SPECIAL = ("zero", "nan", "inf", "tiny", "subnormal")
SENSITIVE = 63                # the mutants of test_dosage_fixed_cpu.py must show from this N and M on


@functools.lru_cache(maxsize=None)
def case(N, M, with_na):
    """the codes, the mask and mu' in code units as the device forms it (left unchanged by every test)"""
    B = gd.codes_matrix(N, M, 8, N * 7 + M)
    m4, na, nonas = gd.na_mask(N, with_na)
    mu = fx.code_mean(B, na)
    for a in (B, m4, na, mu):
        a.setflags(write=False)
    return dict(N=N, M=M, with_na=with_na, B=B, m4=m4, na=na, nonas=nonas, mu=mu)


def host_msig(cs):
    """msig where no device is at hand: the long-double restatement of the statistics, rounded to fp64 (the device's differs from it in
    the last bits; the GPU test takes the device's)"""
    mu, q, _ = gd.ref_code_stats(cs["B"], cs["na"], cs["nonas"])
    return gd.ref_stats(mu, q, cs["nonas"], SCALE, 1.0)[1].astype(np.float64)


def _rng(*key):
    return np.random.default_rng([abs(hash(k)) % (2 ** 31) if isinstance(k, str) else int(k) for k in key])


_KIND_ID = {k: i for i, k in enumerate(KINDS + SPECIAL)}


def _plain(kind, K, seed):
    rng = _rng(K, seed, _KIND_ID[kind])
    v = rng.standard_normal(K)
    if kind == "decades":                 # 12 decades, one dominant entry: most q have empty high digits, small entries are rounded hard
        v = v * 10.0 ** rng.uniform(-12.0, 0.0, K)
        v[K // 3] = 3.7
    elif kind == "zero":
        v[:] = 0.0
    elif kind == "nan":
        v[K // 2] = np.nan
    elif kind == "inf":
        v[K // 2] = -np.inf
    elif kind == "tiny":                  # max|v| < 2^-946: the multiplier is capped at 2^1000; some entries subnormal
        v = v * 2.0 ** -960
        v[1::3] *= 2.0 ** -75
    elif kind == "subnormal":             # subnormal entries beside a normal maximum: q == 0 there
        v[1::4] = rng.integers(-1000, 1000, len(v[1::4])) * 5e-324
    return v


# ---- digit edges ------------------------------------------------------------------------------------------------------------------
RIPPLE = {True: 0x3F7F7F7F7F7F80, False: 0x1F7F7F7F7F7F80}      # digit 0 is -128 and carries, and so on through digit 5: (-128,) * 6 + (64 | 32,)
RIPPLE0 = {True: 0x3EFFFFFFFFFF80, False: 0x1EFFFFFFFFFF80}     # the carry of digit 0 turns every byte 0xFF into a zero digit: (-128, 0 .. 0, 63 | 31)
MAXQ = {True: 2 ** 54 - 2, False: 2 ** 53}                      # the largest |q| a double below 2^e can give; max|v| an exact power of two
TIES = (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -128.5, -129.5, 32767.5, 32768.5)     # on the k + 1/2 grid of the quantiser


def edge_targets(K, top, seed, neg_max):
    """K values t = v 2^(54-e), integers and half-integers (exact doubles): t[0] the maximum; then a carry through all seven digits, the
    ties, digits -128 and +127 in each of the planes 0..5 alone and together (|q| <= 2^54 keeps digit 6 within +-64); the rest random
    integers of every length with ties and the edges again among them.  Returns (t, must): must = how many leading entries only
    serve when they are reached EXACTLY (the others keep their digits under a perturbation of the last bit)"""
    lead = [MAXQ[top], RIPPLE[top], RIPPLE0[top]] + list(TIES)
    must = len(lead)
    rest = ([-MAXQ[top]] if neg_max else []) + [-RIPPLE[top], -RIPPLE0[top]]
    for l in range(6):
        rest += [127 << (8 * l), -(128 << (8 * l))]
    rest += [sum(127 << (8 * l) for l in range(6)), -sum(128 << (8 * l) for l in range(6))]
    L = lead + rest
    rng = _rng(K, seed, int(top), 99)
    t = []
    for i in range(K):
        if i < len(L):
            t.append(L[i])
        elif i % 4 == 0:
            t.append(L[1 + (i // 4) % (len(L) - 1)])
        elif i % 4 == 1:
            t.append(float(rng.integers(-2 ** 30, 2 ** 30)) + 0.5)
        else:
            bits = int(rng.integers(1, 54))
            t.append(int(rng.integers(2 ** (bits - 1), 2 ** bits)) * (1 if rng.random() < 0.5 else -1))
    out = np.array([float(a) for a in t])
    assert all(fx.Fraction(a) == fx.Fraction(float(b)) for a, b in zip(t, out))      # every target is an exact double
    return out, min(must, K)


def p_edge(K, top, seed, e=-25):
    """the digit-edge vector on the ATx side: exact, in a random order"""
    t, _ = edge_targets(K, top, seed, True)
    return np.ldexp(t, e - 54)[_rng(K, seed, 7).permutation(K)]


def solve_weights(c, w):
    """x with fl(w x) == c where a double within two ulps of c / w gives it (reached), c / w elsewhere"""
    x = c / w
    reached = w * x == c
    for direction in (np.inf, -np.inf):
        cand = x
        for _ in range(2):
            cand = np.nextafter(cand, direction)
            ok = ~reached & (w * cand == c)
            x = np.where(ok, cand, x)
            reached = reached | ok
    return x, reached


def x_edge(msig, scale, top, seed, ec=-30):
    """the digit-edge vector on the Ax side: the weights c = msig scale x as the device forms them are to be t 2^(ec-54).  The targets
    that only count when exact (the maximum, the carries, the ties) go to rows where a double x gives them"""
    w = np.asarray(msig, dtype=np.float64) * scale
    M = len(w)
    t, must = edge_targets(M, top, seed, False)
    c = np.ldexp(t, ec - 54)
    order = [int(m) for m in _rng(M, seed, 8).permutation(M)]
    row = np.full(M, -1)
    free = dict.fromkeys(order)
    for i in range(must):
        ok = solve_weights(np.full(M, c[i]), w)[1]
        m = next((m for m in free if ok[m]), next(iter(free)))
        row[i] = m
        del free[m]
    row[must:] = list(free)
    target = np.empty(M)
    target[row] = c
    return solve_weights(target, w)[0]


def p_vector(kind, cs, seed=0):
    """N entries (the caller pads)"""
    N = cs["N"]
    if kind.startswith("edge"):
        return p_edge(N, kind == "edge-top", 11 + seed)
    return _plain(kind, N, 11 + seed)


def x_vector(kind, cs, msig, seed=0):
    M = cs["M"]
    if kind.startswith("edge"):
        return x_edge(msig, SCALE, kind == "edge-top", 23 + seed)
    return _plain(kind, M, 23 + seed)


def weights(msig, x):
    """c = msig scale x as k_dm_max / k_dm_quant form it"""
    return np.asarray(msig, dtype=np.float64) * SCALE * np.asarray(x, dtype=np.float64)


def edge_report(v):
    """what a vector reaches of the digit edges: per plane the extreme digits, carries through all seven digits, entries on the k + 1/2
    grid that ties-to-even and round-half-away send to different integers, the largest |q|, whether max|v| is a power of two"""
    e = fx.exponent(v)
    s = np.asarray(v, dtype=np.float64) * math.ldexp(1.0, 54 - e)
    q = fx.quantise(v, e)
    d = fx.digits(q)                      # (asserts that every q fits 7 balanced digits)
    ripple = (int(np.sum(np.all(d[:6] == -128, axis=0) & (d[6] > 0))),
              int(np.sum((d[0] == -128) & np.all(d[1:6] == 0, axis=0) & (d[6] > 0))))
    ties = int(np.sum((np.abs(s - np.trunc(s)) == 0.5) & (np.rint(s) != np.trunc(s + np.copysign(0.5, s)))))
    return dict(e=e, lo=d.min(axis=1), hi=d.max(axis=1), ripple=ripple, ties=ties, maxq=max(abs(t) for t in q),
                pow2=math.frexp(float(np.max(np.abs(v))))[0] == 0.5)


def assert_edges(rep, top):
    """for K >= SENSITIVE entries"""
    assert np.all(rep["lo"][:6] == -128) and np.all(rep["hi"][:6] == 127), rep
    assert rep["hi"][6] == (64 if top else 32), rep
    assert rep["ripple"][0] >= 1 and rep["ripple"][1] >= 1 and rep["ties"] >= 4, rep
    assert rep["maxq"] == MAXQ[top] and rep["pow2"] == (not top), rep
