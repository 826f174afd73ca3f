"""gv_king_block / gv_king_pairs / gv_king_info against tests/king_restatement.py: the five counts equal as
integers, the kinship BIT-identical (uint64 view, NaN positions included).

Shapes, the smallest at which the kernel can still go wrong: 1003 x 517 (N no multiple of 64 or 256, M no multiple of 64, several
individual groups and K-steps, with hand-placed all-missing / all-heterozygous / duplicate individuals and monomorphic / all-missing
markers), 257 x 65 (one individual in a second 256-block, one marker in a second row group), 5 x 3, 130 x 4200 (66 row groups: the
pipeline's steady state) and the simulated pedigree (67 x 4000)."""
import numpy as np
import pytest

import king_restatement as kr
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
CASES = ("ragged", "edge", "tiny", "deep", "pedigree")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


def _shard(cs, mode=1, layout=2):
    sh = capi.Shard(cs["N"], cs["M"], device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(cs["bed"])            # no mask, no statistics: relatedness is a property of the genotypes
    return sh


def _expect_pairs(cs, cutoff, kin=None, table=None):
    kin = cs["kin"] if kin is None else kin
    table = cs["table"] if table is None else table
    i, j = kr.pairs(kin, cutoff)
    return i, j, kin[i, j], table[i, j]


def _same_pairs(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and kr.same_bits(got[2], want[2])
            and np.array_equal(got[3], want[3]))


@pytest.mark.parametrize("name", CASES)
def test_the_whole_matrix_and_the_pair_list_equal_the_restatement(name):
    cs = kr.case(name)
    N, M = cs["N"], cs["M"]
    with _shard(cs) as sh:
        assert sh.get_layout() == 2
        kin, cnt = sh.king_block(0, N, 0, N)
        assert np.array_equal(cnt, cs["table"])
        assert kr.same_bits(kin, cs["kin"])
        assert kr.same_bits(kin, kin.T)
        info = sh.king_info()
        nG = (N + 63) // 64
        assert info["used_markers"] == M and info["pairs"] == N * N and info["useful_macs"] == 5.0 * M * N * N
        assert info["block_pairs"] == nG * (nG + 1) // 2 and info["scratch_bytes"] > 0 and info["seconds"] > 0
        lists = {}
        for cutoff in (-np.inf, kr.CUT_SECOND, 0.4):
            got = lists[cutoff] = sh.king_pairs(cutoff)
            want = _expect_pairs(cs, cutoff)
            assert _same_pairs(got, want), (name, cutoff, len(got[0]), len(want[0]))
            key = got[0].astype(np.int64) * N + got[1]
            assert np.all(np.diff(key) > 0) and np.all(got[0] < got[1])          # ascending (i, j), i < j
            info = sh.king_info()
            assert info["pairs"] == N * (N - 1) // 2 and info["useful_macs"] == 5.0 * M * (N * (N - 1) // 2)
    if name == "pedigree":
        i, j = np.triu_indices(N, 1)
        rel = cs["truth"][i, j] != kr.UNREL                   # king_pairs(0.0884) returns exactly the related pairs
        assert rel.sum() == 83 and np.array_equal(np.stack(lists[kr.CUT_SECOND][:2]), np.stack([i[rel], j[rel]]))
    if name == "ragged":
        # the hand-placed individuals: all missing -> NaN everywhere; all heterozygous -> 0.5 on the diagonal; a duplicate -> 0.5
        assert np.all(np.isnan(kin[7])) and kin[70, 70] == 0.5 and kin[299, 300] == 0.5 and np.all(cnt[7, :, 0] == 0)


def test_kernel_modes_1_and_2_give_identical_results_and_two_calls_the_same_bytes():
    cs = kr.case("ragged")
    N = cs["N"]
    res = []
    for mode in (1, 2):
        with _shard(cs, mode=mode) as sh:
            assert sh.get_kernel_mode() == mode
            kin, cnt = sh.king_block(0, N, 0, N)
            a, b = sh.king_pairs(0.0), sh.king_pairs(0.0)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            res.append((kin, cnt) + a)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res[0], res[1]))
    assert len(res[0][2]) > 100


def test_rectangles_off_the_64_boundaries_their_mirrors_and_the_diagonal():
    cs = kr.case("ragged")
    N = cs["N"]
    with _shard(cs) as sh:
        for i0, ni, j0, nj in ((3, 70, 130, 61), (60, 10, 60, 10), (0, 1, N - 1, 1), (700, 303, 1, 200), (63, 2, 63, 130), (500, 64, 900, 103),
                               (10, 0, 5, 7)):
            kin, cnt = sh.king_block(i0, ni, j0, nj)
            assert kin.shape == (ni, nj) and cnt.shape == (ni, nj, 5)
            assert kr.same_bits(kin, cs["kin"][i0:i0 + ni, j0:j0 + nj]), (i0, ni, j0, nj)
            assert np.array_equal(cnt, cs["table"][i0:i0 + ni, j0:j0 + nj]), (i0, ni, j0, nj)
            kt, ct = sh.king_block(j0, nj, i0, ni)                                   # the mirror rectangle: the transpose, bit for bit
            assert kr.same_bits(kt, kin.T)
            assert np.array_equal(ct[:, :, [0, 1, 2, 4, 3]], cnt.transpose(1, 0, 2))
        d = np.diag(sh.king_block(0, N, 0, N)[0])
        het = np.diag(cs["counts"]["het_i"])
        assert np.all(d[het > 0] == 0.5) and np.all(np.isnan(d[het == 0])) and (het == 0).any()


def test_use_masks_whose_edges_fall_off_the_4_and_64_marker_boundaries():
    cs = kr.case("ragged")
    N, M = cs["N"], cs["M"]
    masks = []
    u = np.ones(M, dtype=np.uint8)
    u[61:67] = 0
    u[M - 1] = 0
    masks.append(u)
    u = np.zeros(M, dtype=np.uint8)
    u[[2, 63, 64, 255, 256, 515]] = 7                # any non-zero byte counts
    masks.append(u)
    masks.append((np.random.default_rng(5).random(M) < 0.5).astype(np.uint8))
    masks.append(np.zeros(M, dtype=np.uint8))        # nothing used: every count 0, every kinship NaN
    with _shard(cs) as sh:
        for u in masks:
            c = kr.counts(cs["geno"], u)
            kin, cnt = sh.king_block(0, N, 0, N, use=u)
            assert np.array_equal(cnt, kr.table(c))
            assert kr.same_bits(kin, kr.kinship(c))
            assert sh.king_info()["used_markers"] == int((u != 0).sum())
            assert sh.king_info()["useful_macs"] == 5.0 * int((u != 0).sum()) * N * N
            got = sh.king_pairs(kr.CUT_SECOND, use=u)
            assert _same_pairs(got, _expect_pairs(cs, kr.CUT_SECOND, kr.kinship(c), kr.table(c)))
        assert np.all(np.isnan(kin)) and len(got[0]) == 0


def test_a_cap_too_small_reports_the_count_and_cap_zero_works():
    cs = kr.case("edge")
    want = _expect_pairs(cs, 0.0)
    n = len(want[0])
    assert n > 10
    with _shard(cs) as sh:
        for cap in (0, 1, n - 1):
            found, *_ = sh.king_pairs_raw(0.0, cap)                 # return code 0 (no exception), the count right
            assert found == n
        found, pi, pj, kin, cnt = sh.king_pairs_raw(0.0, n)         # exactly enough
        assert found == n and _same_pairs((pi[:n], pj[:n], kin[:n], cnt[:n]), want)
        assert _same_pairs(sh.king_pairs(0.0, cap=3), want)         # the wrapper re-calls once
        found, *_ = sh.king_pairs_raw(0.45, 0)                      # no pair above the cutoff, no slot
        assert found == len(kr.pairs(cs["kin"], 0.45)[0])


def test_a_king_call_leaves_the_products_and_the_ld_scores_of_the_context_unchanged():
    cs = kr.case("ragged")
    N, M = cs["N"], cs["M"]
    rng = np.random.default_rng(9)
    x = rng.standard_normal(M)
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        sh.compute_markers_statistics()
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)
        before = (sh.Ax(x), sh.ATx(p)) + sh.ld_scores(20)
        sh.king_block(5, 100, 300, 50)
        sh.king_pairs(0.1)
        after = (sh.Ax(x), sh.ATx(p)) + sh.ld_scores(20)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


def test_every_refusal_is_raised_with_its_message():
    cs = kr.case("edge")
    N, M = cs["N"], cs["M"]
    with capi.Shard(N, M, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        with pytest.raises(capi.GvError, match="meth"):
            sh.king_block(0, 2, 0, 2)
        with pytest.raises(capi.GvError, match="meth"):
            sh.king_pairs(0.1)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width
        with capi.Shard(N, M, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(N, M, 2, bits).astype(dtype), 1.0 / 127.0)
            with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                sh.king_block(0, 2, 0, 2)
            with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                sh.king_pairs(0.1)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(cs["bed"])
        with pytest.raises(capi.GvError, match="raw rows alone"):
            sh.king_pairs(0.1)
    with _shard(cs, layout=1) as sh:              # two stripe sets: the tile layout is the way out
        assert sh.get_layout() == 1
        with pytest.raises(capi.GvError, match="two stripe sets.*tile layout"):
            sh.king_block(0, 2, 0, 2)
        with pytest.raises(capi.GvError, match="two stripe sets.*tile layout"):
            sh.king_pairs(0.1)
    with _shard(cs) as sh:
        sh.force_multi(1)                         # a job of more than one rank
        with pytest.raises(capi.GvError, match="more than one rank"):
            sh.king_block(0, 2, 0, 2)
        with pytest.raises(capi.GvError, match="more than one rank"):
            sh.king_pairs(0.1)
        sh.force_multi(0)
        for i0, ni, j0, nj in ((-1, 2, 0, 2), (0, N + 1, 0, 1), (N, 1, 0, 1), (0, 1, 250, 8), (0, -1, 0, 1), (0, 1, 0, -1)):
            with pytest.raises(capi.GvError, match="outside"):
                sh.king_block(i0, ni, j0, nj)
        with pytest.raises(capi.GvError, match="cap must not be negative"):
            sh.king_pairs_raw(0.1, -1)
        for bad in (np.nan, np.inf):
            with pytest.raises(capi.GvError, match="cutoff"):
                sh.king_pairs(bad)
        L, i32p, found = sh.L, capi.C.POINTER(capi.C.c_int32), capi.C.c_int64(-7)
        assert L.gv_king_pairs(sh.h, None, 0.1, 4, None, None, None, None, capi.C.byref(found)) != 0      # NULL arrays with cap > 0
        assert b"NULL" in L.gv_last_error(sh.h) and found.value == -7
        assert L.gv_king_pairs(sh.h, None, 0.1, 0, None, None, None, None, None) != 0                     # NULL n_found
        assert b"n_found is NULL" in L.gv_last_error(sh.h)
        assert L.gv_king_info(sh.h, None) != 0 and L.gv_king_block(None, None, 0, 1, 0, 1, None, None) != 0
        assert len(sh.king_pairs(0.1)[0]) == len(kr.pairs(cs["kin"], 0.1)[0])                           # and the context still works
