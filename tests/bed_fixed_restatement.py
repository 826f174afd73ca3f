"""Restatement of the fixed-point products of 2-bit (bed) genotypes -- kernel modes 1 and 2 of include/gvamp.h, DESIGN.md section 4,
the head of gvamp_amd/csrc/gv_mfma.hip -- in Python integers, Fractions and int64 numpy sums, kept apart from the library's code.
Every stage is its own function:

  genotype planes   PLINK 2-bit codes 00 / 10 / 11 / 01 = a 2 / 1 / 0 / missing  ->  r' (2 / 1 / 0, 3 for missing), miss, a' = a if
                    present else 0, b = present; rows of individuals without a phenotype and pad rows are zero.
  operands          Ax, mode 1:  c = fl(msig x),  e = fl(fl(mave - 3) c)         out = sum r' c + sum miss e - K0,  K0 = sum mave c
                    Ax, mode 2:  c = fl(msig x),  e = -fl(mave c)                out = sum a' c + sum b e
                    ATx       :  p itself                                        ONE exponent for c and e together
  quantisation      E with 2^(E-1) <= amax < 2^E;  q = rint(v 2^(54-E)), ties to even;  7 balanced base-256 digits, q = sum d_l 256^l.
                    mode 2 adds the exact residual res = fma(-q, 2^(E-54), v), q2 = rint(res 2^(108-E)); a vector with amax < 2^-915
                    has no second level (2^(108-E) would overflow).  A zero vector has multiplier 0; a non-finite entry makes the
                    result scale NaN, so every output of the product is NaN.
  plane sums        s_l[row] = sum_k plane[row][k] d_l[k], exact (int64 here; asserted to be far inside int64)
  recombination     lo = s0 + s1 2^8 + s2 2^16 + s3 2^24,  hi = s4 + s5 2^8 + s6 2^16,  value = hi 2^32 + lo (integers, exact), then
                    T = fl(fl(hi) 2^32 + fl(lo)):  hi and lo are converted SEPARATELY.
  epilogues         every fp64 rounding in its place, fma through Fraction (one rounding)

"One final rounding".  fl(hi) 2^32 is exact whenever |hi| <= 2^53 (always: |hi| < 2^22 K 384).  fl(lo) is exact while |lo| <= 2^53, and
then T is the exact integer rounded once.  |lo| <= W K 128 (1 + 2^8 + 2^16 + 2^24) with W the largest plane weight of a K-entry, so
fl(lo) can be inexact only past
    ATx, mode 1:  X - 3Y and Y are converted, W = 2 resp. 1 ..... N > 2^53 / (256 * 16 843 009) = 2 088 960 individuals
    Ax,  mode 1:  one plane r' c + miss e, W = 3 + 1 = 4 ......... M > 2^53 / (512 * 16 843 009) = 1 044 480 markers of one shard
    mode 2     :  W = 2 + 1 = 3 (Ax), 2 (ATx)
and only for an adversarial vector (every low digit at -128 and every genotype at the top weight); the digits of real vectors have
random signs, |lo| grows like sqrt(K) and stays ~2^10 below the limit at any size gv_set_dims admits (N 384 < 2^31).  Past the limit
the result carries TWO roundings (fl(lo), then the sum): still within one ulp of the exact integer, but not its correctly rounded
value -- convert() models exactly that, convert(.., "one") is the defective variant that rounds hi 2^32 + lo as one integer.

The scalars K0 = sum mave c (mode-1 Ax) and P = sum p (mode-1 ATx) are ordered fp64 reductions on the device whose bits depend on the
launch shape.  They are FREE INPUTS of the epilogue functions here; exact_K0 / exact_P give them as Fractions, k0_bound / p_bound the
standard summation bound gamma_n sum |term|, and find_scalar (find_K0 / find_P) the procedure that determines EVERY double that
reproduces all output entries.

Domain: amax in [2^-900, 2^900] or zero or non-finite (what the products are used with; outside it powers of two over/underflow)."""
import math
import struct
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)                       # unit roundoff of fp64
WEIGHT = (1 << 0) + (1 << 8) + (1 << 16) + (1 << 24)
VARIANTS = ("", "drop0", "trunc", "one")       # the unmodified restatement and the three defects the tests must be able to see


# ---- genotype planes --------------------------------------------------------------------------------------------------------------
def decode(bed, N, M):
    """M x npad PLINK codes (0..3), npad = 4 ceil(N / 4): individual n of a marker sits at bits 2 (n & 3) of byte n >> 2"""
    mb = (N + 3) // 4
    b = np.asarray(bed, dtype=np.uint8).reshape(M, mb)
    return ((b[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(M, 4 * mb)


def planes(bed, N, M, present=None):
    """dict of M x npad int64 planes r, miss, a, b; zero at pad rows (n >= N) and at individuals without a phenotype"""
    code = decode(bed, N, M)
    npad = code.shape[1]
    keep = np.arange(npad) < N
    if present is not None:
        keep = keep & np.concatenate([np.asarray(present, dtype=bool), np.zeros(npad - N, dtype=bool)])
    a = np.select([code == 0, code == 2, code == 3], [2, 1, 0], 0).astype(np.int64)
    miss = (code == 1).astype(np.int64)
    k = keep.astype(np.int64)[None, :]
    return {"r": (a + 3 * miss) * k, "miss": miss * k, "a": a * k, "b": (1 - miss) * k}


def marker_stats(pl, nonas):
    """mave / msig of data::compute_markers_statistics from the masked planes (float64; the device's last bits may differ: the GPU
    tests take the device's own values, every function below takes them as inputs)"""
    a, b = pl["a"], pl["b"]
    c2, c1, c0 = ((a == 2) & (b == 1)).sum(axis=1), ((a == 1) & (b == 1)).sum(axis=1), ((a == 0) & (b == 1)).sum(axis=1)
    suma, sumb = 2.0 * c2 + c1, (c0 + c1 + c2).astype(np.float64)
    mu = np.where(sumb != 0, suma / np.where(sumb != 0, sumb, 1.0), 0.0)
    ss = c2 * (2.0 - mu) ** 2 + c1 * (1.0 - mu) ** 2 + c0 * mu ** 2
    sg = np.where(ss != 0, 1.0 / np.sqrt(np.where(ss != 0, ss, 1.0) / (nonas - 1.0)), 1.0)
    return mu, sg


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def ax_operands(mode, mave, msig, x):
    """(c, e) of the Ax product, each entry rounded as stated at the top (numpy float64: one IEEE operation per step)"""
    mave, msig, x = (np.asarray(t, dtype=np.float64) for t in (mave, msig, x))
    c = msig * x
    if mode == 1:
        d = mave - 3.0
        return c, d * c
    return c, -(mave * c)


# ---- quantisation -------------------------------------------------------------------------------------------------------------------
def exponent(*vs):
    """E with 2^(E-1) <= amax < 2^E over all the vectors given; None for amax == 0, NaN when an entry is not finite"""
    amax = 0.0
    for v in vs:
        v = np.asarray(v, dtype=np.float64)
        if v.size and not np.all(np.isfinite(v)):
            return math.nan
        if v.size:
            amax = max(amax, float(np.max(np.abs(v))))
    return math.frexp(amax)[1] if amax > 0 else None


def _usable(E):
    return E is not None and not (isinstance(E, float) and math.isnan(E))


def result_scale(E):
    """2^(E-54) as the epilogues use it: 0 for a zero vector, NaN for a non-finite one"""
    if E is None:
        return 0.0
    return math.ldexp(1.0, E - 54) if _usable(E) else math.nan


def quantise(v, E, variant=""):
    """q = rint(v 2^(54-E)) as Python integers, ties to even (round() of a Fraction); all zero when the multiplier is 0"""
    v = np.asarray(v, dtype=np.float64)
    if not _usable(E):
        return [0] * len(v)
    m = Fraction(2) ** (54 - E)
    if variant == "trunc":
        return [int(Fraction(float(t)) * m) for t in v]          # int() of a Fraction truncates towards zero: a defect
    return [round(Fraction(float(t)) * m) for t in v]


def residual_quantise(v, q, E, variant=""):
    """mode 2: q2 = rint((v - q 2^(E-54)) 2^(108-E)); the residual is exact in fp64 (asserted); no second level below 2^-915"""
    if not _usable(E) or E <= -915:
        return [0] * len(q)
    g, m2, out = Fraction(2) ** (E - 54), Fraction(2) ** (108 - E), []
    for t, qq in zip(np.asarray(v, dtype=np.float64), q):
        res = Fraction(float(t)) - qq * g
        assert Fraction(float(res)) == res, "the residual of the head is not a double"
        out.append(int(res * m2) if variant == "trunc" else round(res * m2))
    return out


def digits(q, variant=""):
    """7 x len(q) int64: balanced base-256 digits in [-128, 127], q = sum_l d_l 256^l (asserted)"""
    d = np.zeros((7, len(q)), dtype=np.int64)
    for k, t in enumerate(q):
        for l in range(7):
            dg = ((t + 128) % 256) - 128
            t = (t - dg) // 256
            d[l, k] = dg
        assert t == 0, "q does not fit 7 balanced digits"
    if variant == "drop0":
        d[0] = 0                                                  # the lowest digit column lost: a defect
    return d


# ---- plane sums and recombination -----------------------------------------------------------------------------------------------
def plane_sums(P, d):
    """7 x rows int64: plane l = P @ d_l, P rows x K.  Exact: K * 3 * 128 is asserted to be far below 2^63"""
    P = np.asarray(P, dtype=np.int64)
    assert P.shape[1] * 3 * 128 < 2 ** 62 and int(np.abs(P).max(initial=0)) <= 3
    return np.stack([P @ d[l] for l in range(7)])


def combine(s):
    """(hi, lo) per row as Python integers; the value of a row is hi 2^32 + lo"""
    rows = s.shape[1]
    lo = [int(s[0, r]) + (int(s[1, r]) << 8) + (int(s[2, r]) << 16) + (int(s[3, r]) << 24) for r in range(rows)]
    hi = [int(s[4, r]) + (int(s[5, r]) << 8) + (int(s[6, r]) << 16) for r in range(rows)]
    return hi, lo


def convert(hi, lo, variant=""):
    """fl(fl(hi) 2^32 + fl(lo)): two integer conversions (nearest even), an exact product by 2^32, one rounded sum"""
    if variant == "one":
        return float(hi * 2 ** 32 + lo)                           # hi and lo rounded as ONE integer: a defect past |lo| > 2^53
    return float(Fraction(float(hi)) * 2 ** 32 + Fraction(float(lo)))


def lo_exact(lo):
    """True while fl(lo) is exact for every row"""
    return all(abs(t) <= 2 ** 53 for t in lo)


def fma(a, b, c):
    """a * b + c rounded once"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def post_scale(N):
    """fl(1 / fl(sqrt(N)))"""
    return 1.0 / math.sqrt(float(N))


# ---- the free scalars ---------------------------------------------------------------------------------------------------------------
def exact_K0(mave, c):
    return sum((Fraction(float(m)) * Fraction(float(t)) for m, t in zip(mave, c)), Fraction(0))


def exact_P(p):
    return sum((Fraction(float(t)) for t in p), Fraction(0))


def gamma(n):
    return n * U / (1 - n * U)


def k0_bound(mave, c):
    """gamma_2M sum |mave c|: M additions, and each product is rounded as well (or fused, which is no worse)"""
    return gamma(2 * len(c)) * sum((abs(Fraction(float(m)) * Fraction(float(t))) for m, t in zip(mave, c)), Fraction(0))


def p_bound(p, n):
    """gamma_n sum |p| over the n individuals (the pad slots add exact zeros)"""
    return gamma(n) * sum((abs(Fraction(float(t))) for t in p), Fraction(0))


def ulps(v, exact):
    """distance of the double v from the rational exact, in units of ulp(v)"""
    return float((Fraction(v) - exact) / Fraction(math.ulp(v) if v != 0 else math.ulp(0.0)))


def _key(v):
    """doubles in their order as integers (-0.0 and 0.0 share key 0)"""
    b = struct.unpack("<q", struct.pack("<d", v))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _unkey(k):
    return struct.unpack("<d", struct.pack("<q", k if k >= 0 else (-k) | -0x8000000000000000))[0]


def scalar_interval(f_pin, target, big=2.0 ** 600):
    """[k0, k1): the keys (_key) of the doubles k in [-big, big] with f_pin(k) == target, for f_pin monotone in k (a chain of correctly
    rounded operations is): two bisections over the ordered doubles.  Empty (k0 == k1) when no double reproduces target"""
    lo, hi = _key(-big), _key(big)
    sgn = 1.0 if f_pin(big) >= f_pin(-big) else -1.0

    def first(pred):                                   # the smallest key in [lo, hi + 1] at which pred holds (pred is monotone)
        a, b = lo, hi + 1
        while a < b:
            m = (a + b) // 2
            if pred(sgn * f_pin(_unkey(m))):
                b = m
            else:
                a = m + 1
        return a

    return first(lambda v: v >= sgn * target), first(lambda v: v > sgn * target)


# ---- mode 1 ---------------------------------------------------------------------------------------------------------------------------
def _present_pad(present, N, npad):
    pr = np.ones(N, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    return np.concatenate([pr, np.zeros(npad - N, dtype=bool)])


def ax1_sums(pl, mave, msig, x, variant=""):
    """everything of the mode-1 Ax up to the free scalar: dict with c, e (operands), E, T (npad converted sums, unscaled), hi, lo"""
    c, e = ax_operands(1, mave, msig, x)
    E = exponent(c, e)
    dc, de = digits(quantise(c, E, variant), variant), digits(quantise(e, E, variant), variant)
    s = plane_sums(pl["r"].T, dc) + plane_sums(pl["miss"].T, de)           # the streaming pass keeps the two products in ONE plane
    hi, lo = combine(s)
    return {"c": c, "e": e, "E": E, "hi": hi, "lo": lo, "T": np.array([convert(h, l, variant) for h, l in zip(hi, lo)])}


def ax1_epilogue(S, K0, N, present=None):
    """out[n] = fl(fl(T 2^(E-54) - K0) post) at an individual with a phenotype, 0 elsewhere (the product by 2^(E-54) is exact)"""
    T = S["T"]
    with np.errstate(invalid="ignore"):
        val = (T * result_scale(S["E"]) - K0) * post_scale(N)
    return np.where(_present_pad(present, N, len(T)), val, 0.0)


def atx1_sums(pl, p, N, present=None, variant=""):
    """mode-1 ATx up to the free scalar: sa = fl(X - 3Y) 2^(E-54) (= sum a p), sm = fl(Y) 2^(E-54) (= sum miss p) per marker"""
    p = np.asarray(p, dtype=np.float64)
    gone = ~_present_pad(present, N, len(p))
    assert not np.any(p[gone][np.isfinite(p[gone])] != 0), "p must be zero at NA and pad slots (the contract of ATx)"
    E = exponent(p)
    d = digits(quantise(p, E, variant), variant)
    (xh, xl), (yh, yl) = combine(plane_sums(pl["r"], d)), combine(plane_sums(pl["miss"], d))
    sc = result_scale(E)
    with np.errstate(invalid="ignore"):
        sa = np.array([convert(a - 3 * b, c - 3 * dd, variant) for a, b, c, dd in zip(xh, yh, xl, yl)]) * sc
        sm = np.array([convert(b, dd, variant) for b, dd in zip(yh, yl)]) * sc
    return {"E": E, "sa": sa, "sm": sm, "lo": [c - 3 * dd for c, dd in zip(xl, yl)] + list(yl)}


def atx_finish(core, msig, N):
    """fl(fl(msig core) post)"""
    return np.asarray(msig, dtype=np.float64) * core * post_scale(N)


def atx1_epilogue(S, P, mave, msig, N):
    """out[m] = fl(fl(msig fma(-mave, fl(P - sm), sa)) / sqrt N)"""
    core = np.array([fma(-float(mu), float(P - m_), float(a)) for mu, m_, a in zip(mave, S["sm"], S["sa"])])
    return atx_finish(core, msig, N)


class Run:
    """a run of neighbouring doubles, keys [k0, k1); pinned: how many doubles reproduced the pinning entry alone"""

    def __init__(self, k0, k1, pinned):
        self.k0, self.k1, self.pinned = k0, max(k0, k1), pinned

    @property
    def count(self):
        return self.k1 - self.k0

    def contains(self, v):
        return self.k0 <= _key(v) < self.k1

    def nearest(self, exact):
        """the member closest to the rational exact (None when empty)"""
        if self.count == 0:
            return None
        return _unkey(min(max(_key(float(exact)), self.k0), self.k1 - 1))

    def members(self, cap=64):
        return [_unkey(k) for k in range(self.k0, min(self.k1, self.k0 + cap))]


def find_scalar(one, full, out, pins):
    """The free-scalar procedure.  one(i) = (f, target): entry i of the output as a function of the scalar, and the value it must take;
    full(k): the whole output for scalar k.  Every entry is monotone in the scalar, so the doubles that reproduce entry i form a run
    (scalar_interval) and those that reproduce EVERY entry form the intersection of the runs.  Start from the run of the pinning
    entries; while one of its two ends fails some entry, intersect with the runs of (up to 16 of) the failing entries.  At the end both
    ends reproduce every entry, hence so does everything between them, and nothing outside does: the Run returned is exactly the set of
    doubles for which out == full(k) in every entry (by value: -0.0 == 0.0), possibly empty"""
    out = np.asarray(out, dtype=np.float64)
    k0, k1 = scalar_interval(*one(pins[0]))
    pinned = k1 - k0
    todo = list(pins[1:])
    for _ in range(10000):
        for i in todo:
            a, b = scalar_interval(*one(int(i)))
            k0, k1 = max(k0, a), min(k1, b)
        if k0 >= k1:
            return Run(k0, k0, pinned)
        bad = np.zeros(len(out), dtype=bool)
        for k in {k0, k1 - 1}:
            bad |= np.asarray(full(_unkey(k)), dtype=np.float64) != out
        todo = list(np.nonzero(bad)[0][:16])
        if not todo:
            return Run(k0, k1, pinned)
    raise AssertionError("find_scalar does not converge")


def find_K0(S, out, N, present=None):
    """the procedure for the mode-1 Ax.  The pinning entry is the individual with a phenotype whose output is smallest in magnitude
    (and not zero): there T - K0 is smallest against K0, which pins K0 tightest"""
    pr = _present_pad(present, N, len(out))
    idx = np.nonzero(pr & (out != 0))[0]
    n0 = int(idx[np.argmin(np.abs(out[idx]))])
    sc, post = result_scale(S["E"]), post_scale(N)

    def one(n):
        ts = float(S["T"][n]) * sc
        return (lambda k: (ts - k) * post) if pr[n] else (lambda k: 0.0), float(out[n])

    return find_scalar(one, lambda k: ax1_epilogue(S, k, N, present), out, [n0])


def find_P(S, out, mave, msig, N, pin, lm=None):
    """the procedure for the mode-1 ATx; the pinning entry is marker `pin` (the monomorphic one: mave = 2, msig = 1, sm = 0, so
    out sqrt(N) = sa - 2 P up to rounding); lm = (tau, gam2, x): out is lmmse_mult's.  (Where P is small against the sums over the
    missing genotypes -- p = Ax(x) adds up to ~0 -- fl(P - sm) absorbs it at every marker but the monomorphic one, and in lmmse_mult
    tau r vanishes against gam2 x there as well: the run of P that reproduces every entry is then long, and still exact.)"""
    mave, msig = np.asarray(mave, dtype=np.float64), np.asarray(msig, dtype=np.float64)

    def full(P, sl=slice(None)):
        r = atx1_epilogue({"sa": S["sa"][sl], "sm": S["sm"][sl]}, P, mave[sl], msig[sl], N)
        return r if lm is None else lmmse(lm[0], r, lm[1], np.asarray(lm[2], dtype=np.float64)[sl])

    def one(m):
        return (lambda P: float(full(P, slice(m, m + 1))[0]), float(out[m]))

    return find_scalar(one, full, out, [pin])


# ---- mode 2 ---------------------------------------------------------------------------------------------------------------------------
def two_level(head_s, res_s, E, variant="", parts=None):
    """fl(fl(H) 2^(E-54) + fl(R) 2^(E-108)) per row: both products exact, one rounded sum (parts: a list that receives (head, res))"""
    (hh, hl), (rh, rl) = combine(head_s), combine(res_s)
    sc = result_scale(E)
    with np.errstate(invalid="ignore"):
        head = np.array([convert(a, b, variant) for a, b in zip(hh, hl)]) * sc
        res = np.array([convert(a, b, variant) for a, b in zip(rh, rl)]) * (sc * 2.0 ** -54)
        if parts is not None:
            parts.append((head, res))
        return head + res


def _levels(v, E, variant):
    q = quantise(v, E, variant)
    return digits(q, variant), digits(residual_quantise(v, q, E, variant), variant)


def ax2(pl, mave, msig, x, N, present=None, variant="", parts=None):
    """mode-2 Ax: out[n] = fl(two_level post) at an individual with a phenotype, 0 elsewhere"""
    c, e = ax_operands(2, mave, msig, x)
    E = exponent(c, e)
    (dc, dc2), (de, de2) = _levels(c, E, variant), _levels(e, E, variant)
    A, B = pl["a"].T, pl["b"].T
    val = two_level(plane_sums(A, dc) + plane_sums(B, de), plane_sums(A, dc2) + plane_sums(B, de2), E, variant, parts) * post_scale(N)
    return np.where(_present_pad(present, N, len(val)), val, 0.0)


def atx2(pl, mave, msig, p, N, present=None, variant="", parts=None):
    """mode-2 ATx: out[m] = fl(fl(msig fma(-mave, sb, sa)) / sqrt N), sa / sb the two-level sums over the a' / b planes"""
    p = np.asarray(p, dtype=np.float64)
    gone = ~_present_pad(present, N, len(p))
    assert not np.any(p[gone][np.isfinite(p[gone])] != 0), "p must be zero at NA and pad slots (the contract of ATx)"
    E = exponent(p)
    d, d2 = _levels(p, E, variant)
    sa = two_level(plane_sums(pl["a"], d), plane_sums(pl["a"], d2), E, variant, parts)
    sb = two_level(plane_sums(pl["b"], d), plane_sums(pl["b"], d2), E, variant, parts)
    if parts is not None:
        parts.append((sa, sb))
    core = np.array([fma(-float(mu), float(b), float(a)) for mu, a, b in zip(mave, sa, sb)])
    return atx_finish(core, msig, N)


def lmmse(tau, r, gam2, x):
    """fma(tau, r, fl(gam2 x)) per marker"""
    g = gam2 * np.asarray(x, dtype=np.float64)
    return np.array([fma(float(tau), float(a), float(b)) for a, b in zip(r, g)])


# ---- the inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------
SHAPES = {"ragged": dict(N=1003, M=517, fna=0.02, seed=41), "even": dict(N=2100, M=1100, fna=0.0, seed=43)}
MONO, ALLMISS = 70, 133                     # markers made monomorphic (every genotype a = 2) and all-missing


def case(name):
    """N, M, bed, the phenotype mask (present, mask4 or None, nonas) of one shape: ~1 % missing genotypes, one monomorphic and one
    all-missing marker, ~2 % individuals without a phenotype on the ragged shape"""
    from gvamp_amd import synth
    sp = SHAPES[name]
    N, M = sp["N"], sp["M"]
    mb = (N + 3) // 4
    bed = synth.synth_bed(N, M, seed=sp["seed"], miss_ppm=10000).reshape(M, mb).copy()
    bed[MONO], bed[ALLMISS] = 0x00, 0x55
    present, m4 = np.ones(N, dtype=bool), None
    if sp["fna"] > 0 or N % 4:
        present = np.random.default_rng(sp["seed"]).random(N) >= sp["fna"]
        m4 = np.zeros(mb, dtype=np.uint8)
        idx = np.nonzero(present)[0]
        np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return dict(name=name, N=N, M=M, npad=4 * mb, bed=bed.reshape(-1), present=present, m4=m4, nonas=int(present.sum()))


def _solve(fn, target, guess, span=48):
    up = dn = float(guess)
    for _ in range(span):
        if fn(up) == target:
            return up
        if fn(dn) == target:
            return dn
        up, dn = math.nextafter(up, math.inf), math.nextafter(dn, -math.inf)
    return None


def _specials(E):
    """operand values that probe the quantiser at exponent E (grid g = 2^(E-54)): exact ties of both parities and signs, one high up,
    just below / at / just above the flush threshold g / 2 = 2^(E-55), far below it, and -0.0"""
    g = math.ldexp(1.0, E - 54)
    ties = [(j + 0.5) * g for j in (0, 1, 2, 3)] + [-(j + 0.5) * g for j in (0, 1, 2, 3)] + [(2.0 ** 40 + 0.5) * g, (2.0 ** 40 + 1.5) * g]
    edge = [math.nextafter(0.5, 0.0) * g, math.nextafter(0.5, 1.0) * g, -math.nextafter(0.5, 0.0) * g, math.ldexp(1.0, E - 60)]
    return ties + edge + [-0.0]


def vector_p(cs, kind):
    """the N-space vector of `kind` 1..4 (npad doubles, zero at NA and pad slots)"""
    N, npad, pres = cs["N"], cs["npad"], cs["present"]
    rng = np.random.default_rng(1000 + kind + cs["M"])
    p = np.zeros(npad)
    if kind == 1:
        p[:N] = rng.standard_normal(N)
    elif kind == 2:
        p[:N] = rng.standard_normal(N) * 10.0 ** rng.uniform(-12, 0, N)
    elif kind == 3:
        A = 8.0                                              # amax = 2^3: E = 4
        p[:N] = rng.standard_normal(N) * 0.5
        sp = [A, -A, A * (1 - 2.0 ** -53)] + _specials(4)
        slots = np.nonzero(pres)[0][5::7][:len(sp)]
        assert len(slots) == len(sp)
        p[slots] = sp
    p[:N] *= pres
    if kind == 3:
        assert exponent(p) == 4 and np.max(np.abs(p)) == 8.0
    return p


def vector_x(cs, kind, mode, mave, msig):
    """the M-space vector of `kind` 1..4.  kind 3 is built for the operands of `mode`: x[MONO] = 2^10 gives c = 2^10 and e = -2^10
    (mode 1: mave - 3 = -1, msig = 1 there) or -2^11 (mode 2), the power-of-two amax; the predecessor of amax is an e-value and the
    probes of _specials are c-values at ordinary markers, each found by nudging x until the operand comes out exactly"""
    M = cs["M"]
    rng = np.random.default_rng(2000 + kind + cs["N"])
    if kind == 1:
        return rng.standard_normal(M)
    if kind == 2:
        return rng.standard_normal(M) * 10.0 ** rng.uniform(-12, 0, M)
    if kind == 4:
        return np.zeros(M)
    assert mave[MONO] == 2.0 and msig[MONO] == 1.0
    x = rng.standard_normal(M) * 0.25
    x[MONO] = 1024.0
    E = 11 if mode == 1 else 12
    amax = math.ldexp(1.0, E - 1)

    def ops(i, v):
        c, e = ax_operands(mode, mave[i:i + 1], msig[i:i + 1], np.array([v]))
        return float(c[0]), float(e[0])

    free = [i for i in range(3, M) if i not in (MONO, ALLMISS) and msig[i] != 1.0]
    targets = [("e", -amax * (1 - 2.0 ** -53))] + [("c", t) for t in _specials(E)]
    for which, t in targets:
        for i in free:
            if t == 0:
                got = -0.0
            else:
                d = (float(mave[i]) - 3.0 if mode == 1 else -float(mave[i])) if which == "e" else 1.0
                f = float(msig[i]) * d
                # (an e-value near amax needs |e / c| > 1, or c itself would pass amax)
                got = _solve(lambda v: ops(i, v)[which == "e"], t, t / f) if (which == "c" or abs(d) > 1.0) else None
            if got is not None:
                x[i] = got
                free.remove(i)
                break
        else:
            raise AssertionError("no marker takes the operand value %r" % (t,))
    c, e = ax_operands(mode, mave, msig, x)
    assert exponent(c, e) == E and max(np.max(np.abs(c)), np.max(np.abs(e))) == amax
    return x
