"""Dense numpy restatement of the pairwise kinship (gv_king_block / gv_king_pairs), written from the definition in
include/gvamp.h and not from the kernel: genotypes decoded from the .bed bytes, the five counts as int64 matrix products of the planes
P, H, D, then ibs0, d2 and kin with exactly the two fp64 operations of the contract.  Also the simulated pedigree the tests classify.
Test infrastructure only."""
import numpy as np

_CODE = {2: 0, 1: 2, 0: 3, -1: 1}      # allele count (-1 = missing) -> PLINK 2-bit code
_ALLELE = np.array([2, -1, 1, 0], dtype=np.int8)      # PLINK 2-bit code -> allele count


def encode(geno):
    """M * ceil(N/4) marker-major PLINK bytes of an N x M matrix of allele counts 0 / 1 / 2, -1 = missing"""
    geno = np.asarray(geno)
    N, M = geno.shape
    mb = (N + 3) // 4
    codes = np.zeros((M, 4 * mb), dtype=np.uint8)
    for g, c in _CODE.items():
        codes[:, :N][geno.T == g] = c
    c4 = codes.reshape(M, mb, 4)
    return (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8).reshape(-1)


def decode(bed, N, M):
    """N x M allele counts (-1 = missing) from the marker-major .bed bytes (without the three magic bytes)"""
    mb = (N + 3) // 4
    b = np.asarray(bed, dtype=np.uint8).reshape(M, mb)
    codes = np.stack([(b >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(M, 4 * mb)[:, :N]
    return _ALLELE[codes].T.astype(np.int64)


def counts(geno, use=None):
    """dict of the N x N int64 matrices nsnp, hethet, het_i, het_j, dd, ibs0, d2; [i][j]: het_i is the row individual's"""
    a = np.asarray(geno, dtype=np.int64)
    u = np.ones(a.shape[1], dtype=np.int64) if use is None else (np.asarray(use) != 0).astype(np.int64)
    P = (a >= 0).astype(np.int64) * u[None, :]
    H = (a == 1).astype(np.int64) * P
    D = (a - 1) * P
    nsnp, hethet, het_i, het_j, dd = P @ P.T, H @ H.T, H @ P.T, P @ H.T, D @ D.T
    homhom = nsnp - het_i - het_j + hethet
    assert np.all((homhom - dd) % 2 == 0)
    ibs0 = (homhom - dd) // 2
    d2 = 4 * ibs0 + (het_i - hethet) + (het_j - hethet)
    return dict(nsnp=nsnp, hethet=hethet, het_i=het_i, het_j=het_j, dd=dd, ibs0=ibs0, d2=d2)


def kinship(c):
    """kin = 0.5 - (double)d2 / (double)(4 mn), mn = min(het_i, het_j); NaN where mn == 0"""
    mn = np.minimum(c["het_i"], c["het_j"])
    num, den = c["d2"].astype(np.float64), (4 * mn).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = num / np.where(mn == 0, 1.0, den)
    return np.where(mn == 0, np.nan, 0.5 - q)


def table(c):
    """N x N x 5 int32 in the order of the C ABI: nsnp, hethet, ibs0, het_i, het_j"""
    return np.stack([c["nsnp"], c["hethet"], c["ibs0"], c["het_i"], c["het_j"]], axis=2).astype(np.int32)


def pairs(kin, cutoff):
    """(i, j) of every pair i < j with kin >= cutoff, ascending"""
    N = kin.shape[0]
    i, j = np.triu_indices(N, 1)
    with np.errstate(invalid="ignore"):
        keep = kin[i, j] >= cutoff
    return i[keep].astype(np.int32), j[keep].astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def random_geno(N, M, seed, miss=0.05):
    """allele counts from per-marker frequencies uniform in 0.05 .. 0.5, a fraction `miss` of them missing"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, M)
    g = (rng.random((N, M)) < f[None, :]).astype(np.int64) + (rng.random((N, M)) < f[None, :]).astype(np.int64)
    g[rng.random((N, M)) < miss] = -1
    return g


# ---- the simulated pedigree ----------------------------------------------------------------------------------------------------------
# 40 founders; 8 families: two siblings of founders (2f, 2f + 1), a mate (founder 16 + f) of the first sibling, their child -- the second
# sibling's niece or nephew and the first founders' grandchild; 3 duplicates of founders 30, 31, 32: N = 40 + 8 * 3 + 3 = 67.
DUP, FIRST, SECOND, UNREL = 3, 1, 2, 0
CUT_DUP, CUT_FIRST, CUT_SECOND = 0.354, 0.177, 0.0884
PED_SEED, PED_M, PED_FOUNDERS, PED_FAMILIES, PED_DUPS, PED_MISS = 20261020, 4000, 40, 8, 3, 0.05


def pedigree():
    """(geno N x M with -1 = missing, truth N x N of DUP / FIRST / SECOND / UNREL)"""
    rng = np.random.default_rng(PED_SEED)
    M = PED_M
    f = rng.uniform(0.1, 0.5, M)
    hap = (rng.random((PED_FOUNDERS, 2, M)) < f[None, None, :]).astype(np.int64)      # two haplotypes per founder

    def child(pa, pb):
        # unlinked markers: each parent passes one of its two alleles, independently per marker
        sa, sb = rng.integers(0, 2, M), rng.integers(0, 2, M)
        return np.stack([np.where(sa == 0, pa[0], pa[1]), np.where(sb == 0, pb[0], pb[1])])

    people = [hap[i] for i in range(PED_FOUNDERS)]
    rel = {}
    for fam in range(PED_FAMILIES):
        pa, pb, mate = 2 * fam, 2 * fam + 1, 16 + fam
        s1, s2 = len(people), len(people) + 1
        people.append(child(hap[pa], hap[pb]))
        people.append(child(hap[pa], hap[pb]))
        g = len(people)
        people.append(child(people[s1], hap[mate]))
        for p in (pa, pb):
            rel[(p, s1)] = rel[(p, s2)] = FIRST
            rel[(p, g)] = SECOND                      # grandparent
        rel[(s1, s2)] = FIRST
        rel[(s1, g)] = rel[(mate, g)] = FIRST
        rel[(s2, g)] = SECOND                         # aunt or uncle
    for k in range(PED_DUPS):
        src = 30 + k
        rel[(src, len(people))] = DUP
        people.append(people[src].copy())
    geno = np.stack([p[0] + p[1] for p in people])
    N = geno.shape[0]
    geno[rng.random((N, M)) < PED_MISS] = -1
    truth = np.zeros((N, N), dtype=np.int64)
    for (x, y), r in rel.items():
        truth[x, y] = truth[y, x] = r
    return geno, truth


def classify(kin):
    """the class of every kinship value by the usual cutoffs (NaN: unrelated)"""
    with np.errstate(invalid="ignore"):
        return np.where(kin >= CUT_DUP, DUP, np.where(kin >= CUT_FIRST, FIRST, np.where(kin >= CUT_SECOND, SECOND, UNREL)))


_CACHE = {}


def case(name):
    """shared, read-only inputs and references of the GPU tests: dict N, M, geno, bed, counts, kin, table"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "pedigree":
        geno, truth = pedigree()
    else:
        N, M, seed = {"ragged": (1003, 517, 11), "edge": (257, 65, 12), "tiny": (5, 3, 13), "deep": (130, 4200, 14)}[name]
        geno, truth = random_geno(N, M, seed), None
        if name == "ragged":
            # hand-placed: an all-missing individual, an all-heterozygous one, a duplicate, monomorphic and all-missing markers
            geno[:, 5] = 0
            geno[:, 130] = 2
            geno[:, 200] = -1
            geno[7, :] = -1
            geno[70, :] = 1
            geno[300, :] = geno[299, :]
    c = counts(geno)
    out = dict(N=geno.shape[0], M=geno.shape[1], geno=geno, bed=encode(geno), counts=c, kin=kinship(c), table=table(c), truth=truth)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[name] = out
    return out
