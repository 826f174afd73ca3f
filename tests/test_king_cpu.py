"""The restatement of the pairwise kinship (tests/king_restatement.py) held to a brute-force count, to hand cases and to a simulated
pedigree.  No GPU: this is what the GPU tests of gv_king_block / gv_king_pairs are then held to."""
import numpy as np

import king_restatement as kr


def test_the_matrix_products_equal_a_double_loop_over_pairs():
    N, M = 40, 300
    g = kr.random_geno(N, M, seed=1, miss=0.05)
    assert (g < 0).any()
    assert np.array_equal(kr.decode(kr.encode(g), N, M), g)
    c = kr.counts(g)
    kin = kr.kinship(c)
    for i in range(N):
        for j in range(N):
            both = (g[i] >= 0) & (g[j] >= 0)
            a, b = g[i][both], g[j][both]
            nsnp, het_i, het_j = int(both.sum()), int((a == 1).sum()), int((b == 1).sum())
            hethet = int(((a == 1) & (b == 1)).sum())
            ibs0 = int((((a == 0) & (b == 2)) | ((a == 2) & (b == 0))).sum())         # opposite homozygotes
            d2 = int(((a - b) ** 2).sum())                                            # the sum of squared differences
            got = tuple(int(c[k][i, j]) for k in ("nsnp", "hethet", "het_i", "het_j", "ibs0", "d2"))
            assert got == (nsnp, hethet, het_i, het_j, ibs0, d2), (i, j)
            mn = min(het_i, het_j)
            want = np.float64(0.5) - np.float64(d2) / np.float64(4 * mn) if mn else np.nan
            assert kr.same_bits(kin[i, j], want), (i, j)
    assert kr.same_bits(kin, kin.T)


def test_hand_cases():
    g = kr.random_geno(12, 200, seed=2, miss=0.1)
    g[3] = g[2]                                   # a duplicate, missing entries included
    g[5][g[5] == 1] = 0                           # no heterozygote
    g[6] = -1                                     # all missing
    kin = kr.kinship(kr.counts(g))
    assert kin[2, 3] == 0.5 and kin[3, 2] == 0.5
    assert np.all(np.diag(kin)[[0, 1, 2, 3, 4]] == 0.5)
    assert np.all(np.isnan(kin[5])) and np.all(np.isnan(kin[:, 5]))
    assert np.all(np.isnan(kin[6])) and np.all(kr.counts(g)["nsnp"][6] == 0)
    i, j = kr.pairs(kin, -np.inf)                 # a NaN never passes a cutoff
    assert 5 not in i and 5 not in j and 6 not in i and 6 not in j and len(i) == 10 * 9 // 2
    # a use mask equals deleting the markers
    use = (np.arange(200) % 3 != 1).astype(np.uint8)
    a, b = kr.counts(g, use), kr.counts(g[:, use != 0])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert kr.same_bits(kr.kinship(a), kr.kinship(b))


def test_the_simulated_pedigree_is_classified_without_error():
    cs = kr.case("pedigree")
    N = cs["N"]
    assert N == 67 and cs["M"] == 4000
    i, j = np.triu_indices(N, 1)
    assert len(i) == 2211
    kin, truth = cs["kin"][i, j], cs["truth"][i, j]
    for cls, name in ((kr.DUP, "duplicate"), (kr.FIRST, "first degree"), (kr.SECOND, "second degree"), (kr.UNREL, "unrelated")):
        k = kin[truth == cls]
        print("%s: %d pairs, kinship %.4f .. %.4f" % (name, k.size, k.min(), k.max()))
    assert (truth == kr.DUP).sum() == 3 and (truth == kr.FIRST).sum() == 8 * 7 and (truth == kr.SECOND).sum() == 8 * 3
    assert np.array_equal(kr.classify(kin), truth)
    pi, pj = kr.pairs(cs["kin"], kr.CUT_SECOND)
    assert np.array_equal(np.stack([pi, pj]), np.stack([i[truth != kr.UNREL], j[truth != kr.UNREL]]))
