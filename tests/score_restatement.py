"""numpy / rational restatement of the host-side pieces of the scoring batch: the column builder of
gvamp_amd/csrc/host/score_cols.hpp and the plan of gvamp_amd/csrc/gv_score_plan.h."""
from fractions import Fraction  # noqa: F401 (re-exported for the tests)

import numpy as np

SEG_MARKERS_MAX = (2 ** 31 - 1) // 512          # 4 194 303: a K-entry adds up to 512 to an int32 digit sum
MAX_KS = 64
PREP_BLOCKS_MAX = 1024


def allele_to_std(w, msig, sqrtN):
    """x_j = fl(fl(w_j sqrtN) / msig_j)"""
    return (np.asarray(w, dtype=np.float64) * np.float64(sqrtN)) / np.asarray(msig, dtype=np.float64)


def fma(a, b, c):
    """a * b + c rounded once (finite arguments)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def allele_constant(w, mave):
    """K <- fma(mave_j, w_j, K) in marker order"""
    k = 0.0
    for m, t in zip(mave, w):
        k = fma(m, t, k)
    return k


def threshold_columns(w0, index_of, p, thresholds):
    w0, index_of, p = np.asarray(w0, dtype=np.float64), np.asarray(index_of, dtype=np.int64), np.asarray(p, dtype=np.float64)
    own = index_of == np.arange(len(w0))
    with np.errstate(invalid="ignore"):
        return [np.where(own & (p <= t), w0, 0.0) for t in thresholds]


def dense_allele_score(code, w, present_markers_mean):
    """S_n = sum_j w_j a~_nj on mean-imputed allele counts: code is M x N PLINK codes (0: a = 2, 2: a = 1, 3: a = 0, 1: missing)"""
    a = np.array([2.0, np.nan, 1.0, 0.0])[code]
    a = np.where(np.isnan(a), np.asarray(present_markers_mean)[:, None], a)
    return np.asarray(w, dtype=np.float64) @ a


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def up256(x):
    return (x + 255) // 256 * 256


def cp_for(n, cp):
    w = 4
    while w < cp:
        if n <= w:
            return w
        w *= 2
    return cp


def seg_markers(k0, k1, M):
    return max(min(k1 * 64, M) - k0 * 64, 0)


def bounds(nkb, ks):
    return [nkb * j // ks for j in range(ks + 1)]


def bound_ok(nkb, ks, M):
    if not (1 <= ks <= MAX_KS and ks <= nkb):
        return False
    b = bounds(nkb, ks)
    return max(seg_markers(b[j], b[j + 1], M) for j in range(ks)) <= SEG_MARKERS_MAX


def min_ks(nkb, M):
    ks = max(-(-M // SEG_MARKERS_MAX), 1)
    while ks <= MAX_KS and ks <= nkb:
        if bound_ok(nkb, ks, M):
            return ks
        ks += 1
    return 0


def plan(N, M, C, cp, ks_pin, fill):
    """dict as gvs::make_plan fills gvs::Plan; err as there"""
    nrg, nkb = -(-N // 256), -(-M // 64)
    mk = min_ks(nkb, M)
    if not mk:
        return dict(err=2)
    if ks_pin > 0:
        ks = min(ks_pin, nkb)
        if not bound_ok(nkb, ks, M):
            return dict(err=1)
    else:
        ks = max(min(-(-fill // nrg), max(nkb // 8, 1), MAX_KS), mk)
        while ks <= MAX_KS and not bound_ok(nkb, ks, M):
            ks += 1
        if ks > MAX_KS:
            return dict(err=2)
    cpp = cp_for(C, cp)
    passes = -(-C // cpp)
    dig, part = up256(nkb * cpp * 1024), up256(ks * cpp * 256 * nrg * 32)
    small = up256(cpp * (4 + 2 * PREP_BLOCKS_MAX) * 8)
    return dict(err=0, cp=cpp, cp_last=cp_for(C - (passes - 1) * cpp, cpp), passes=passes, ks=ks, min_ks=mk, nrg=nrg, nkb=nkb,
                items=nrg * ks, b=bounds(nkb, ks), dig=dig, part=part, small=small, scratch=dig + part + small)
