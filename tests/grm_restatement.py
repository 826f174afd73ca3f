"""Dense numpy restatement of the standardised genetic relationship matrix (gv_grm_weights / gv_grm_block / gv_grm_pairs, DESIGN.md
section 28), written from the definition in include/gvamp.h and not from the kernel: per-marker integers n, s; the three fp64 weight
operations; Z; S = Z Z^T; the exact common-marker counts; A = S / M_ij with NaN where M_ij = 0.  Also |Z| |Z|^T, which the tests' error
bound is stated in.  Genotype coding, random genotypes and the simulated pedigree are those of tests/king_restatement.py.
Test infrastructure only."""
import numpy as np

import king_restatement as kr

CUT_DUP, CUT_FIRST, CUT_SECOND = 0.7, 0.3, 0.1          # A is twice a kinship: duplicates 1, first degree 1/2, second degree 1/4


def weights(geno, use=None):
    """(mu[M], rs[M], counting[M] bool, dropped: selected markers that do not count) -- n and s in exact integers, then
    mu = s / n, h = mu (1 - 0.5 mu), rs = 1 / sqrt(h), each one correctly rounded fp64 operation"""
    g = np.asarray(geno, dtype=np.int64)
    M = g.shape[1]
    on = np.ones(M, dtype=bool) if use is None else (np.asarray(use) != 0)
    present = g >= 0
    n = present.sum(axis=0)
    s = np.where(present, g, 0).sum(axis=0)
    counting = on & (n > 0) & (s > 0) & (s < 2 * n)
    mu, rs = np.zeros(M), np.zeros(M)
    c = counting
    mu[c] = s[c].astype(np.float64) / n[c].astype(np.float64)
    h = mu[c] * (1.0 - 0.5 * mu[c])
    rs[c] = 1.0 / np.sqrt(h)
    return mu, rs, counting, int((on & ~counting).sum())


def grm(geno, use=None):
    """dict mu, rs, counting, dropped, Z, S, M_ij (int64), A, absS of an N x M matrix of allele counts (-1 = missing)"""
    g = np.asarray(geno, dtype=np.int64)
    mu, rs, counting, dropped = weights(g, use)
    live = (g >= 0) & counting[None, :]
    Z = np.where(live, (g.astype(np.float64) - mu[None, :]) * rs[None, :], 0.0)
    P = live.astype(np.int64)
    S = Z @ Z.T
    absS = np.abs(Z) @ np.abs(Z).T
    Mij = P @ P.T
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(Mij > 0, S / np.where(Mij > 0, Mij, 1).astype(np.float64), np.nan)
    return dict(mu=mu, rs=rs, counting=counting, dropped=dropped, Z=Z, S=S, M_ij=Mij, A=A, absS=absS)


def bound(r):
    """the entry-wise error bound of the tests: (M_ij + 16) 2^-53 absS_ij / M_ij -- an M_ij-term fp64 sum in any order (M_ij u per unit of
    sum |z z|), plus the roundings of the two z (4 u) and of the division (1 u), with room to 16; 0 where M_ij = 0"""
    m = r["M_ij"].astype(np.float64)
    return np.where(m > 0, (m + 16.0) * 2.0 ** -53 * r["absS"] / np.where(m > 0, m, 1.0), 0.0)


def within(got, r, ref=None, bnd=None):
    """got against the restatement: NaN exactly where the reference has it, elsewhere within the bound"""
    ref = r["A"] if ref is None else ref
    bnd = bound(r) if bnd is None else bnd
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(np.all(np.abs(got[~nan] - ref[~nan]) <= bnd[~nan]))


def pairs(A, cutoff):
    """(i, j) of every pair i < j with A >= cutoff, ascending"""
    return kr.pairs(A, cutoff)


def near(r, cutoff):
    """N x N bool: the reference value is within the entry's bound of the cutoff, so the pair may fall on either side"""
    with np.errstate(invalid="ignore"):
        return np.abs(r["A"] - cutoff) <= bound(r)


def brute(geno, use=None):
    """(A, M_ij) by a double loop over pairs and a Python loop over markers: slow, for small shapes"""
    g = np.asarray(geno, dtype=np.int64)
    N, M = g.shape
    mu, rs, counting, _ = weights(g, use)
    A, Mij = np.full((N, N), np.nan), np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        for j in range(N):
            s, m = 0.0, 0
            for k in range(M):
                if counting[k] and g[i, k] >= 0 and g[j, k] >= 0:
                    s += ((float(g[i, k]) - mu[k]) * rs[k]) * ((float(g[j, k]) - mu[k]) * rs[k])
                    m += 1
            Mij[i, j] = m
            if m:
                A[i, j] = s / float(m)
    return A, Mij


# the hand-placed features of `ragged`
MISSING_IND, DUP_A, DUP_B = 7, 299, 300
MONO0, MONO2, ALLMISS, SINGLETON, SINGLETON_IND = 5, 130, 200, 400, 10

_SHAPES = {"ragged": (1003, 517, 11), "edge": (257, 65, 12), "tiny": (5, 3, 13), "deep": (130, 4200, 14)}
CASES = ("ragged", "edge", "tiny", "deep", "pedigree")
_CACHE = {}


def case(name):
    """shared, read-only inputs and references of the tests: dict N, M, geno, bed, truth and the entries of grm()"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "pedigree":
        geno, truth = kr.pedigree()
    else:
        N, M, seed = _SHAPES[name]
        geno, truth = kr.random_geno(N, M, seed), None
        if name == "ragged":
            # the row edits first, the marker edits after them, so that the markers keep what they were made for
            geno[MISSING_IND, :] = -1
            geno[DUP_B, :] = geno[DUP_A, :]
            geno[geno[:, MONO0] >= 0, MONO0] = 0             # all present genotypes 0
            geno[geno[:, MONO2] >= 0, MONO2] = 2             # all present genotypes 2
            geno[:, ALLMISS] = -1                            # missing in everyone
            geno[geno[:, SINGLETON] >= 0, SINGLETON] = 0     # one heterozygote among the present: the largest |z|
            geno[SINGLETON_IND, SINGLETON] = 1
    out = dict(N=geno.shape[0], M=geno.shape[1], geno=geno, bed=kr.encode(geno), truth=truth)
    out.update(grm(geno))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[name] = out
    return out
