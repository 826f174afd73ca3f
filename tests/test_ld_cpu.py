"""The numpy restatement of the LD scores (tests/ld_restatement.py) held to independent routes: np.corrcoef on complete data, the
A^T A route through the standardised matrix, and the band, chromosome, monomorphic and adjusted rules on small hand cases.  No GPU."""
import numpy as np

from gvamp_amd import synth
import ld_restatement as ldr
import precond_restatement as pr


def _host(bed, N, M, na=None):
    a, b = pr.decode(bed, N, M)
    na = np.ones(N) if na is None else na
    mave, msig = pr.marker_stats(a, b, na)
    return a, b, na, mave, msig


def test_complete_data_equals_corrcoef():
    N, M = 700, 150
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=0, ld_block=48, ld_ppm=900000)
    a, b, na, mave, msig = _host(bed, N, M)
    assert np.all(b == 1)
    r, poly = ldr.corr(ldr.gram(a, b, na, mave, msig))
    assert poly.all()
    assert np.max(np.abs(r - np.corrcoef(a.T))) <= 1e-12
    assert np.max(np.abs(r - np.eye(M))) > 0.5          # the blocks are correlated: the comparison is not of zeros


def test_gram_equals_the_matrix_route_with_missing_and_mask():
    N, M = 603, 130
    bed = synth.synth_bed(N, M, seed=5, miss_ppm=20000, S=11, ld_block=48, ld_ppm=900000)
    na = np.ones(N)
    na[::7] = 0.0
    a, b, na, mave, msig = _host(bed, N, M, na)
    A = pr.matrix(a, b, na, mave, msig)
    G = A.T @ A
    C = ldr.gram(a, b, na, mave, msig)
    assert np.max(np.abs(C - G)) <= 1e-12 * np.max(np.diag(G))
    assert np.array_equal(C, C.T)
    r, poly = ldr.corr(C)
    assert np.array_equal(r, r.T) and np.all(np.diag(r)[poly] == 1.0)
    d = np.sqrt(np.diag(G))
    assert np.max(np.abs(r - G / np.outer(d, d))) <= 1e-12


def test_band_chromosome_and_monomorphic_rules():
    rng = np.random.default_rng(1)
    N, M, B = 40, 9, 2
    g = rng.integers(0, 3, size=(N, M))
    g[:, 3] = 1              # constant
    g[:, 6] = -1             # missing everywhere
    g[5, 0] = -1
    res = ldr.ld(ldr.encode(g), N, M, B)
    r, poly = res["r"], res["poly"]
    assert list(poly) == [True, True, True, False, True, True, False, True, True]
    assert np.all(r[3] == 0) and np.all(r[:, 6] == 0) and r[3, 3] == 0 and r[0, 0] == 1
    assert np.isnan(res["l2"][[3, 6]]).all() and np.all(res["npairs"][[3, 6]] == 0)
    # marker 4: band {2, 3, 4, 5, 6}, 3 and 6 monomorphic
    assert res["npairs"][4] == 3 and abs(res["l2"][4] - (1 + r[4, 2] ** 2 + r[4, 5] ** 2)) <= 1e-15
    assert res["npairs"][0] == 3 and res["npairs"][8] == 2     # clipped at the ends; 8's band holds 6 (monomorphic) and 7
    chrom = [1, 1, 1, 1, 1, 2, 2, 2, 2]
    l2, n = ldr.scores(r, poly, B, chrom)
    assert n[4] == 2 and abs(l2[4] - (1 + r[4, 2] ** 2)) <= 1e-15          # 5 is on the next chromosome
    assert n[5] == 2 and abs(l2[5] - (1 + r[5, 7] ** 2)) <= 1e-15
    bd = ldr.band(r, B, 3, 4, chrom)
    assert bd.shape == (4, 5)
    assert bd[1, 2] == 1 and bd[1, 0] == r[4, 2] and bd[1, 1] == 0 and bd[1, 3] == 0 and bd[1, 4] == 0
    assert bd[2, 2] == 1 and bd[2, 0] == 0 and bd[2, 1] == 0 and bd[2, 4] == r[5, 7]
    full = ldr.band(r, B, 0, M)
    assert full[0, 0] == 0 and full[0, 1] == 0 and full[M - 1, 4] == 0 and full[0, 4] == r[0, 2]


def test_adjusted_score_on_a_hand_computed_case():
    # deviations from the mean 1: x1 = (-1, 0, 1, -1, 0, 1), x2 = (-1, 0, 1, 0, -1, 1), x3 = (1, 0, -1, -1, 0, 1); every sum of squares
    # is 4, the cross sums are 3, 0, -1: r12 = 3/4, r13 = 0, r23 = -1/4.  n = 6: f(x) = x - (1 - x) / 4.
    g = np.array([[0, 0, 2], [1, 1, 1], [2, 2, 0], [0, 1, 0], [1, 0, 1], [2, 2, 2]])
    res = ldr.ld(ldr.encode(g), 6, 3, 2)
    assert np.max(np.abs(res["r"] - np.array([[1, .75, 0], [.75, 1, -.25], [0, -.25, 1]]))) <= 1e-15
    assert np.max(np.abs(res["l2"] - np.array([1.5625, 1.625, 1.0625]))) <= 1e-15
    adj = ldr.ld(ldr.encode(g), 6, 3, 2, adjusted=True)
    assert np.max(np.abs(adj["l2"] - np.array([1.203125, 1.28125, 0.578125]))) <= 1e-15
    assert list(adj["npairs"]) == [3, 3, 3]
    one = ldr.ld(ldr.encode(g), 6, 3, 1, adjusted=True)        # window 1: markers 1 and 3 lose each other
    assert np.max(np.abs(one["l2"] - np.array([1.453125, 1.28125, 0.828125]))) <= 1e-15
    assert list(one["npairs"]) == [2, 3, 2]


def test_masked_individuals_do_not_count():
    # a marker whose only missing genotypes sit at masked individuals behaves as a complete marker on the others
    rng = np.random.default_rng(2)
    N, M = 60, 5
    g = rng.integers(0, 3, size=(N, M))
    na = np.ones(N)
    na[::5] = 0.0
    g2 = g.copy()
    g2[::5, 2] = -1
    r1 = ldr.ld(ldr.encode(g), N, M, 4, na=na)
    r2 = ldr.ld(ldr.encode(g2), N, M, 4, na=na)
    assert np.array_equal(r1["r"], r2["r"]) and np.array_equal(r1["l2"], r2["l2"])
    keep = na == 1
    assert np.max(np.abs(r1["r"] - np.corrcoef(g[keep].T))) <= 1e-12
