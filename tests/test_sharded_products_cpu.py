"""The fixtures of the sharded-product tests can do their job (no GPU): tests/sharded_products.py is what tests/test_gpu_sharded_products.py
and tests/test_gpu_sharded_drivers.py compare with, so every comparison in it is shown here to fail on the defect it is there for.

* every split tiles [0, Mt); `even2` is the oracle's divide_work;
* the offset arithmetic c * Mt + S reproduces the one-rank layout, and a shard whose S is off by one does not;
* the bit comparisons see one ulp, the sign of a zero and a NaN payload, in one entry of one rank;
* the float64 restatement of Z = A W deviates from the long-double one by more than 0 on the library inputs: the 16 x bound of the GPU
  test is a measured figure above nothing, and the figure is printed;
* the clump index has a member on each side of a shard edge and an index marker that opens a shard, for two and for three ranks, and the
  shard-local rule of the driver selects the markers of the global rule (dropping the map to local indices does not)."""
import numpy as np
import pytest

import bed_fixed_restatement as bx
import sharded_products as sp

MT_DRIVER = 10000                             # the toy data of tests/test_gpu_sharded_drivers.py


@pytest.mark.parametrize("name", list(sp.splits()))
def test_every_split_tiles_the_markers(name):
    split = sp.splits()[name]
    assert sp.tiles_exactly(split, sp.MT), split
    assert [sp.owner(split, m) for m in (0, sp.MT - 1)] == [0, len(split) - 1]
    # a gap, an overlap and a short cover are seen
    S, M = split[-1]
    assert not sp.tiles_exactly(split[:-1] + [(S + 1, M - 1)], sp.MT)
    assert not sp.tiles_exactly(split[:-1] + [(S - 1, M + 1)], sp.MT)
    assert not sp.tiles_exactly(split[:-1] + [(S, M - 1)], sp.MT)


def test_the_named_shards_are_the_ones_the_issue_is_about(oracle):
    s = sp.splits()
    assert s["even2"] == [(0, 259), (259, 258)]
    assert [(S, M) for M, S in (oracle.divide_work(sp.MT, 2, r) for r in range(2))] == s["even2"]
    for n in (2, 3, 5, 8):
        assert [(S, M) for M, S in (oracle.divide_work(MT_DRIVER, n, r) for r in range(n))] == sp.divide_work(MT_DRIVER, n)
    assert s["uneven3"] == [(0, 1), (1, 64), (65, 452)] and s["empty3"][1] == (300, 0)
    assert s["uneven3"][0][1] < 10                                  # fewer markers than the PCA block of the `ragged` case


@pytest.mark.parametrize("name", list(sp.splits()))
def test_slabs_written_at_c_mt_plus_s_are_the_one_rank_file(name):
    split, Mt, C = sp.splits()[name], sp.MT, 9
    rng = np.random.default_rng(5)
    full = rng.standard_normal((C, Mt))
    full[2, 70], full[3, 133], full[4, 0] = np.nan, -0.0, np.inf
    parts = [full[:, S:S + M] for S, M in split]
    sp.assert_concatenation_is_the_one_shard_result(split, Mt, parts, full, name)
    assert sp.assemble(split, Mt, parts).size == C * Mt
    # one shard's S off by one value, either way: seen (the last shard cannot move up, the first not down)
    for r, (S, M) in enumerate(split):
        if M == 0:
            continue
        for d in (-1, 1):
            if S + d < 0 or S + M + d > Mt:
                continue
            moved = sp.assemble(split, Mt, parts, shift={r: d})
            assert sp.first_bit_difference(moved, sp.one_rank_layout(full)) is not None, (name, r, d)
            with pytest.raises(AssertionError):
                assert sp.same_bits(moved, sp.one_rank_layout(full))
    # a column stride of the shard's M in place of Mt: seen
    wrong = np.zeros(C * Mt)
    for S, M in split:
        for c in range(C):
            wrong[c * M + S:c * M + S + M] = full[c, S:S + M]
    assert not sp.same_bits(wrong, sp.one_rank_layout(full))


def test_the_bit_comparisons_see_one_ulp_a_signed_zero_and_a_nan_payload():
    rng = np.random.default_rng(6)
    a = rng.standard_normal((3, 40))
    a[1, 5], a[2, 7] = np.nan, 0.0
    ranks = [a.copy() for _ in range(3)]
    sp.assert_same_on_every_rank(ranks, "copies")
    for edit in ("ulp", "zero", "payload"):
        b = a.copy()
        if edit == "ulp":
            b[0, 3] = np.nextafter(b[0, 3], np.inf)
        elif edit == "zero":
            b[2, 7] = -0.0
        else:
            b.view(np.uint64)[1, 5] ^= np.uint64(1)                 # still a NaN, another payload
            assert np.isnan(b[1, 5]) and np.array_equal(a, b, equal_nan=True)
        assert not sp.same_bits(a, b) and sp.first_bit_difference(a, b) is not None, edit
        with pytest.raises(AssertionError):
            sp.assert_same_on_every_rank([a, a.copy(), b], edit)
    # an eigenvalue one ulp off on one rank
    ev = [np.array([3.25, 1.5]) for _ in range(3)]
    ev[2][1] = np.nextafter(ev[2][1], 0.0)
    with pytest.raises(AssertionError):
        sp.assert_same_on_every_rank(ev, "eval")
    assert not sp.same_bits(np.zeros(3), np.zeros(4))


def test_the_float64_restatement_of_the_score_deviates_from_long_double():
    cs = bx.case("ragged")
    N, M = cs["N"], cs["M"]
    mave, msig = bx.marker_stats(bx.planes(cs["bed"], N, M, cs["present"]), cs["nonas"])
    W = sp.score_columns(cs, mave, msig)
    assert W.shape == (9, M) and not W[3].any() and not W[7].any() and W[8].any()
    A, A64 = sp.dense_A(cs["bed"], N, M, cs["present"]), sp.dense_A(cs["bed"], N, M, cs["present"], dtype=np.float64)
    assert A.dtype == np.longdouble and A64.dtype == np.float64 and np.finfo(np.longdouble).eps < 2.0 ** -60
    assert np.all(A[~cs["present"]] == 0) and np.all(A[:, [bx.MONO, bx.ALLMISS]] == 0)
    ref, r64 = sp.dense_score(A, W), sp.dense_score(A64, W)
    dev64, per = sp.score_deviation(r64, ref)
    print("float64 restatement of A W against long double, N = %d, M = %d: deviation %.3e (per column %s); bound of the GPU test %.3e"
          % (N, M, dev64, " ".join("%.1e" % d for d in per), sp.score_bound(dev64)))
    assert 0.0 < dev64 < 1e-13
    assert per[3] == 0.0 and per[7] == 0.0                          # the zero columns
    # the deviation sees what it is for: one entry moved by 1e-11 of its column, and a zero column that is not zero
    bad = np.array(r64)
    bad[0, 11] += 1e-11 * np.max(np.abs(ref[0]))
    assert sp.score_deviation(bad, ref)[0] > sp.score_bound(dev64)
    bad = np.array(r64)
    bad[3, 0] = 1e-300
    assert sp.score_deviation(bad, ref)[0] == float("inf")
    # a shard left out of the sum is far outside the bound
    S, Mh = sp.splits()["even2"][1]
    part = sp.dense_score(A64[:, :S], W[:, :S])
    assert sp.score_deviation(part, ref)[0] > 1e-3


@pytest.mark.parametrize("n", [2, 3])
def test_the_clump_index_crosses_the_shard_edges(n):
    idx, p, w0, thr = sp.clump_fixture(MT_DRIVER)
    split = sp.divide_work(MT_DRIVER, n)
    assert idx.shape == p.shape == w0.shape == (MT_DRIVER,)
    # a well-formed index file: every member names an index marker
    for j, g in enumerate(idx):
        assert g == -1 or (g == int(g) and idx[int(g)] == g), (j, g)
    cross = sp.cross_shard_members(idx, split)
    firsts = sp.shard_first_index_markers(idx, split)
    assert firsts == [S for S, _ in split[1:]]
    below = [(j, g) for j, g in cross if j < g]
    above = [(j, g) for j, g in cross if j > g]
    assert below and above, cross                                   # an index marker in the shard above its member, and one below
    for S, _ in split[1:]:
        assert (S - 1, S) in cross and (S + 3, S - 5) in cross
    # those markers are loud and under every threshold
    for j, g in cross:
        if abs(j - g) <= 8 and any(abs(j - S) <= 5 for S, _ in split[1:]):
            assert abs(w0[j]) >= 1000.0 and p[j] < thr[0] and abs(w0[g]) >= 1000.0 and p[g] < thr[0]
    for t in thr:
        want = sp.used_markers_global(idx, p, t)
        got = sp.used_markers_sharded(idx, p, t, split)
        assert np.array_equal(np.sort(got), want) and len(want) > 20
        assert all(S in want for S in firsts)                       # the shard-first index markers are used ...
        assert not any(j in want for j, _ in cross)                 # ... and no member is, wherever its index marker lives
    assert 7 in sp.used_markers_global(idx, p, 0.01) and 7 not in sp.used_markers_global(idx, p, 0.001)
    # the defect: the global index compared with the shard-local position selects nothing beyond the first shard
    naive = [S + j for S, M in split for j in range(M) if idx[S + j] == j and p[S + j] <= thr[2]]
    assert not np.array_equal(np.sort(naive), sp.used_markers_global(idx, p, thr[2]))
