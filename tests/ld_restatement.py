"""Dense numpy restatement of the LD scores and banded LD correlations (gv_ld_scores / gv_ld_band), written
from the definitions in include/gvamp.h on top of precond_restatement's PLINK decode and marker statistics: the Gram entries from
the integer planes, the correlation with its monomorphic rule, the band with its chromosome rule, the LD score raw and adjusted.
Test infrastructure only."""
import numpy as np

import precond_restatement as pr

_CODE = {2: 0, 1: 2, 0: 3, -1: 1}      # genotype (-1 = missing) -> PLINK 2-bit code


def encode(geno):
    """M * ceil(N/4) marker-major PLINK bytes of an N x M matrix of genotypes 0 / 1 / 2, -1 = missing"""
    geno = np.asarray(geno)
    N, M = geno.shape
    mb = (N + 3) // 4
    codes = np.zeros((M, 4 * mb), dtype=np.uint8)
    for g, c in _CODE.items():
        codes[:, :N][geno.T == g] = c
    c4 = codes.reshape(M, mb, 4)
    return (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8).reshape(-1)


def gram(a, b, na, mave, msig):
    """C_jk = msig_j msig_k / N (VV_jk - mave_k VP_jk - mave_j VP_kj + mave_j mave_k PP_jk) from the integer sums of the planes
    P = b na, V = a P; evaluated for j <= k and mirrored"""
    N = a.shape[0]
    P = (b * na[:, None]).astype(np.int64)
    V = a.astype(np.int64) * P
    VV, VP, PP = (V.T @ V).astype(np.float64), (V.T @ P).astype(np.float64), (P.T @ P).astype(np.float64)
    inner = VV - mave[None, :] * VP - mave[:, None] * VP.T + np.outer(mave, mave) * PP
    C = np.outer(msig, msig) * (1.0 / N) * inner
    U = np.triu(C)
    return U + np.triu(C, 1).T


def corr(C):
    """r_jk = C_jk / sqrt(C_jj C_kk); r_jj = 1 for a polymorphic marker; 0 wherever a marker is monomorphic (C_jj == 0)"""
    d = np.diag(C).copy()
    poly = d != 0
    den = np.sqrt(np.outer(d, d))
    r = np.where(np.outer(poly, poly), C / np.where(den != 0, den, 1.0), 0.0)
    r[np.diag_indices_from(r)] = poly.astype(np.float64)
    return r, poly


def in_band(M, B, chrom=None):
    """M x M booleans: |j - k| <= B and, with chrom, the same chromosome"""
    j = np.arange(M)
    ok = np.abs(j[:, None] - j[None, :]) <= B
    if chrom is not None:
        ch = np.asarray(chrom)
        ok &= ch[:, None] == ch[None, :]
    return ok


def scores(r, poly, B, chrom=None, adjusted=False, nonas=None):
    """(l2, npairs): l_j = 1 + sum_{k != j in band, k polymorphic} f(r_jk^2), NaN for a monomorphic j; npairs counts the terms, self
    included, 0 for a monomorphic j"""
    M = r.shape[0]
    terms = in_band(M, B, chrom) & poly[None, :] & ~np.eye(M, dtype=bool)
    x = r * r
    f = x - (1.0 - x) / (nonas - 2.0) if adjusted else x
    l2 = 1.0 + np.where(terms, f, 0.0).sum(1)
    n = 1.0 + terms.sum(1)
    return np.where(poly, l2, np.nan), np.where(poly, n, 0.0)


def band(r, B, j0, nj, chrom=None):
    """nj x (2B + 1): column B + d of row j - j0 is r[j][j + d], 0 outside the band"""
    M = r.shape[0]
    rb = np.where(in_band(M, B, chrom), r, 0.0)
    out = np.zeros((nj, 2 * B + 1))
    for d in range(-B, B + 1):
        j = np.arange(max(j0, -d), min(j0 + nj, M - d))
        if j.size:
            out[j - j0, B + d] = rb[j, j + d]
    return out


def ld(bed, N, M, B, na=None, chrom=None, adjusted=False):
    """everything from the bytes: dict of r (M x M, unbanded), poly, l2, npairs"""
    a, b = pr.decode(bed, N, M)
    na = np.ones(N) if na is None else na
    mave, msig = pr.marker_stats(a, b, na)
    r, poly = corr(gram(a, b, na, mave, msig))
    l2, n = scores(r, poly, B, chrom, adjusted, float(na.sum()))
    return {"r": r, "poly": poly, "l2": l2, "npairs": n}
