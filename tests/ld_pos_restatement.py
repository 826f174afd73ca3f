"""Dense numpy restatement of the positional, annotation-partitioned LD scores (gv_ld_scores_pos), written from
the definition in include/gvamp.h on top of ld_restatement: the band from positions and chromosomes by brute force, the scores per
category, the last in-band index of every marker, and the block count of the launch restated from it.  Test infrastructure only."""
import numpy as np

LD_WINDOW_MAX = 8192


def in_band_pos(pos, radius, chrom=None):
    """M x M booleans, brute force: the same chromosome and, for j <= k, the fp64 expression pos[k] - pos[j] <= radius; mirrored"""
    pos = np.asarray(pos, dtype=np.float64)
    M = pos.size
    up = (pos[None, :] - pos[:, None]) <= radius          # [j][k]: pos_k - pos_j
    up = np.triu(up)
    ok = up | up.T
    if chrom is not None:
        ch = np.asarray(chrom)
        ok &= ch[:, None] == ch[None, :]
    return ok


def window_hi(pos, radius, chrom=None, rows=512):
    """hi[j]: the last index k >= j in the band of j, looking at every k (no monotonicity assumed); a few rows at a time so that the
    largest reach (8192) fits"""
    pos = np.asarray(pos, dtype=np.float64)
    M = pos.size
    ch = None if chrom is None else np.asarray(chrom)
    hi = np.zeros(M, dtype=np.int64)
    k = np.arange(M)
    for j0 in range(0, M, rows):
        j = np.arange(j0, min(j0 + rows, M))
        ok = ((pos[None, :] - pos[j, None]) <= radius) & (k[None, :] >= j[:, None])
        if ch is not None:
            ok &= ch[None, :] == ch[j, None]
        hi[j] = np.where(ok, k[None, :], -1).max(1)
    return hi


def dmax_of(hi):
    """the most row groups a 64-marker row group reaches ahead"""
    M = hi.size
    return max(int(hi[min(64 * I + 63, M - 1)]) // 64 - I for I in range((M + 63) // 64))


def block_pairs(hi):
    """blocks (I, J >= I) of 64 x 64 markers that hold an in-band pair: what the launch computes, the others return at once"""
    M = hi.size
    return sum(int(hi[min(64 * I + 63, M - 1)]) // 64 - I + 1 for I in range((M + 63) // 64))


def entries(pos, radius, chrom=None):
    """sum over j of hi_j - lo_j + 1, the (j, k) entries of the band, self included"""
    return int(in_band_pos(pos, radius, chrom).sum())


def scores_pos(r, poly, pos, radius, chrom=None, adjusted=False, nonas=None, annot=None, scale=False):
    """(l2, npairs): l(j, c) = a_jc + sum_{k != j in band, k polymorphic} f(r_jk^2) a_kc, NaN for a monomorphic j; npairs counts the
    terms, self included, 0 for a monomorphic j.  l2 is (M,) without annot (a = 1), (M, C) with it.  scale=True returns a third
    array, |a_jc| + sum |f| |a_kc|: the magnitude an entry's rounding error is held against."""
    M = r.shape[0]
    terms = in_band_pos(pos, radius, chrom) & poly[None, :] & ~np.eye(M, dtype=bool)
    x = r * r
    f = x - (1.0 - x) / (nonas - 2.0) if adjusted else x
    A = np.ones((M, 1)) if annot is None else np.asarray(annot, dtype=np.float64)
    l2 = np.empty((M, A.shape[1]))
    mag = np.empty((M, A.shape[1]))
    for c in range(A.shape[1]):           # (the sum of ld_restatement.scores, term by term: a ones column gives its bits)
        l2[:, c] = A[:, c] + np.where(terms, f * A[None, :, c], 0.0).sum(1)
        mag[:, c] = np.abs(A[:, c]) + np.where(terms, np.abs(f) * np.abs(A[None, :, c]), 0.0).sum(1)
    n = 1.0 + terms.sum(1)
    l2 = np.where(poly[:, None], l2, np.nan)
    if annot is None:
        l2, mag = l2[:, 0], mag[:, 0]
    out = (l2, np.where(poly, n, 0.0))
    return out + (mag,) if scale else out
