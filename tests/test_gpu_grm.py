"""gv_grm_weights / gv_grm_block / gv_grm_pairs / gv_grm_info against tests/grm_restatement.py: the weights
BIT-identical (uint64 view), the common-marker counts equal as integers, NaN positions identical and every entry within

    |A - A_ref|_ij <= (M_ij + 16) 2^-53 absS_ij / M_ij,      absS = |Z| |Z|^T

which is derived, not measured: the standard bound of an M_ij-term fp64 sum in ANY order (M_ij u per unit of sum |z_i z_j|), plus the
roundings of the two z (4 u) and of the division (1 u), with room to 16.  Symmetry, rectangles, pair lists and repeated calls are held
bit for bit against the library's own whole-matrix call.

Shapes, the smallest at which the kernel can still go wrong: 1003 x 517 (N no multiple of 64 or 256, M no multiple of 64 or 4, several
individual groups and row groups, with hand-placed monomorphic / all-missing / singleton markers, an all-missing individual and a
duplicate pair), 257 x 65 (one individual in a second 256-block, one marker in a second row group), 5 x 3, 130 x 4200 (66 row groups:
the loop's steady state) and the simulated pedigree (67 x 4000)."""
import numpy as np
import pytest

import grm_restatement as gr
import king_restatement as kr
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
CASES = gr.CASES
CUTOFFS = (-np.inf, 0.1, 0.7)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


def _shard(cs, mode=1, layout=2, bed=None, M=None):
    sh = capi.Shard(cs["N"], cs["M"] if M is None else M, device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(cs["bed"] if bed is None else bed)            # no mask, no statistics: relatedness is a property of the genotypes
    return sh


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_WHOLE = {}


def _whole(name):
    """the library's whole matrix of a case, computed once and shared read-only: (a, m_common)"""
    if name not in _WHOLE:
        cs = gr.case(name)
        with _shard(cs) as sh:
            a, mc = sh.grm_block(0, cs["N"], 0, cs["N"])
        a.setflags(write=False)
        mc.setflags(write=False)
        _WHOLE[name] = (a, mc)
    return _WHOLE[name]


@pytest.mark.parametrize("name", CASES)
def test_the_weights_are_bit_identical_to_the_restatement(name):
    cs = gr.case(name)
    with _shard(cs) as sh:
        mu, rs, n_used = sh.grm_weights()
        info = sh.grm_info()
    assert np.array_equal(_bits(mu), _bits(cs["mu"])), np.flatnonzero(_bits(mu) != _bits(cs["mu"]))[:5]
    assert np.array_equal(_bits(rs), _bits(cs["rs"])), np.flatnonzero(_bits(rs) != _bits(cs["rs"]))[:5]
    assert n_used == int(cs["counting"].sum()) == info["counting_markers"] and info["dropped_markers"] == cs["dropped"]
    assert info["pairs"] == 0 and info["useful_macs"] == 0 and info["block_pairs"] == 0 and info["scratch_bytes"] > 0
    if name == "ragged":
        assert cs["dropped"] == 3 and rs[gr.SINGLETON] == rs.max()


@pytest.mark.parametrize("name", CASES)
def test_the_whole_matrix_is_within_the_derived_bound_of_the_restatement(name):
    cs = gr.case(name)
    N = cs["N"]
    a, mc = _whole(name)
    assert np.array_equal(mc, cs["M_ij"])
    assert np.array_equal(np.isnan(a), np.isnan(cs["A"]))
    ok = ~np.isnan(cs["A"])
    err, bnd = np.abs(a - cs["A"])[ok], gr.bound(cs)[ok]
    print(name, "largest error / bound:", float((err / bnd).max()) if ok.any() else None)
    assert np.all(err <= bnd)
    assert np.array_equal(_bits(a), _bits(a.T))
    assert a.shape == (N, N)
    if name == "ragged":
        m, da, db = gr.MISSING_IND, gr.DUP_A, gr.DUP_B
        assert np.all(np.isnan(a[m])) and np.all(np.isnan(a[:, m])) and np.all(mc[m] == 0)
        b = gr.bound(cs)
        assert abs(a[da, db] - a[da, da]) <= b[da, db] and abs(a[da, db] - a[db, db]) <= b[da, db] and mc[da, db] == mc[da, da]


def test_rectangles_off_the_64_boundaries_their_mirrors_and_the_diagonal():
    cs = gr.case("ragged")
    N = cs["N"]
    a, mc = _whole("ragged")
    with _shard(cs) as sh:
        for i0, ni, j0, nj in ((3, 70, 130, 61), (60, 10, 60, 10), (0, 1, N - 1, 1), (700, 303, 1, 200), (63, 2, 63, 130), (500, 64, 900, 103),
                               (10, 0, 5, 7)):
            ra, rm = sh.grm_block(i0, ni, j0, nj)
            assert ra.shape == (ni, nj) and rm.shape == (ni, nj)
            assert np.array_equal(_bits(ra), _bits(a[i0:i0 + ni, j0:j0 + nj])), (i0, ni, j0, nj)
            assert np.array_equal(rm, mc[i0:i0 + ni, j0:j0 + nj]), (i0, ni, j0, nj)
            ta, tm = sh.grm_block(j0, nj, i0, ni)                                    # the mirror rectangle: the transpose, bit for bit
            assert np.array_equal(_bits(ta), _bits(ra.T)) and np.array_equal(tm, rm.T)
            info = sh.grm_info()
            assert info["pairs"] == ni * nj and info["useful_macs"] == float(info["counting_markers"]) * ni * nj
        d = np.diag(sh.grm_block(0, N, 0, N)[0])
        assert np.array_equal(_bits(d), _bits(np.diag(a)))
        assert np.isnan(d[gr.MISSING_IND]) and np.isfinite(np.delete(d, gr.MISSING_IND)).all()


def test_use_masks_whose_edges_fall_off_the_4_and_64_marker_boundaries():
    cs = gr.case("ragged")
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
    with _shard(cs) as sh:
        for u in masks:
            r = gr.grm(cs["geno"], u)
            a, mc = sh.grm_block(0, N, 0, N, use=u)
            assert np.array_equal(mc, r["M_ij"]) and gr.within(a, r)
            info = sh.grm_info()
            assert info["counting_markers"] == int(r["counting"].sum()) and info["dropped_markers"] == r["dropped"]
            mu, rs, n_used = sh.grm_weights(use=u)
            assert np.array_equal(_bits(mu), _bits(r["mu"])) and np.array_equal(_bits(rs), _bits(r["rs"])) and n_used == r["counting"].sum()
            keep = u != 0
            with _shard(cs, bed=kr.encode(cs["geno"][:, keep]), M=int(keep.sum())) as cut:      # the same markers, deleted
                ca, cm = cut.grm_block(0, N, 0, N)
            assert np.array_equal(cm, mc) and gr.within(ca, r, ref=a)
            got = sh.grm_pairs(0.1, use=u)
            _check_list(got, r, 0.1, N)
        u = np.zeros(M, dtype=np.uint8)              # nothing selected: every count 0, every value NaN, no pair
        a, mc = sh.grm_block(0, N, 0, N, use=u)
        assert np.all(np.isnan(a)) and not mc.any() and len(sh.grm_pairs(-np.inf, use=u)[0]) == 0
        assert sh.grm_info()["counting_markers"] == 0 and sh.grm_info()["dropped_markers"] == 0


def _check_list(got, r, cutoff, N):
    """a delivered pair list against the restatement r: ascending (i, j), i < j; the (i, j) set equal except where the reference value
    is within the entry's bound of the cutoff, and those fewer than 1 % of the list; values within the bound, counts exact"""
    pi, pj, a, mc = got[:4]
    key = pi.astype(np.int64) * N + pj
    assert np.all(np.diff(key) > 0) and np.all(pi < pj)
    wi, wj = gr.pairs(r["A"], cutoff)
    wkey = wi.astype(np.int64) * N + wj
    odd = np.setxor1d(key, wkey)
    near = gr.near(r, cutoff) if np.isfinite(cutoff) else np.zeros((N, N), dtype=bool)
    assert np.all(near[odd // N, odd % N]), (cutoff, len(odd))
    iu, ju = np.triu_indices(N, 1)
    assert near[iu, ju].sum() * 100 < max(len(wkey), 1) or near[iu, ju].sum() == 0
    assert np.array_equal(mc, r["M_ij"][pi, pj])
    assert np.all(np.abs(a - r["A"][pi, pj]) <= gr.bound(r)[pi, pj])
    assert not np.isnan(a).any()


@pytest.mark.parametrize("name", CASES)
def test_the_pair_lists_equal_the_restatement_and_the_whole_matrix(name):
    cs = gr.case(name)
    N = cs["N"]
    a, mc = _whole(name)
    lists = {}
    with _shard(cs) as sh:
        for cutoff in CUTOFFS:
            got = lists[cutoff] = sh.grm_pairs(cutoff)
            _check_list(got, cs, cutoff, N)
            pi, pj = got[0], got[1]
            assert np.array_equal(_bits(got[2]), _bits(a[pi, pj])) and np.array_equal(got[3], mc[pi, pj])       # the same bits by either road
            assert np.array_equal(_bits(got[4]), _bits(np.diag(a))) and np.array_equal(got[5], np.diag(mc))     # the diagonal
            again = sh.grm_pairs(cutoff)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
            info = sh.grm_info()
            nG = (N + 63) // 64
            assert info["pairs"] == N * (N - 1) // 2 and info["block_pairs"] == nG * (nG + 1) // 2
            assert info["counting_markers"] == int(cs["counting"].sum()) and info["dropped_markers"] == cs["dropped"]
            assert info["useful_macs"] == float(info["counting_markers"]) * (N * (N - 1) // 2)
            assert info["scratch_bytes"] > 0 and info["seconds"] > 0
        nodiag = sh.grm_pairs(0.1, diag=False)
        assert nodiag[4] is None and nodiag[5] is None and all(x.tobytes() == y.tobytes() for x, y in zip(nodiag[:4], lists[0.1][:4]))
    if name == "pedigree":
        i, j = np.triu_indices(N, 1)
        rel = cs["truth"][i, j] != kr.UNREL                   # grm_pairs(0.1) returns exactly the related pairs
        assert rel.sum() == 83 and np.array_equal(np.stack(lists[0.1][:2]), np.stack([i[rel], j[rel]]))
        assert len(lists[0.7][0]) == 3


def test_a_cap_too_small_reports_the_count_and_cap_zero_works():
    cs = gr.case("edge")
    N = cs["N"]
    a, mc = _whole("edge")
    wi, wj = gr.pairs(a, 0.0)                       # (the library's own values decide: the list is held to the matrix bit for bit)
    n = len(wi)
    assert n > 10
    with _shard(cs) as sh:
        for cap in (0, 1, n - 1):
            found, *rest = sh.grm_pairs_raw(0.0, cap)               # return code 0 (no exception), the count right
            assert found == n
            assert np.array_equal(_bits(rest[4]), _bits(np.diag(a))) and np.array_equal(rest[5], np.diag(mc))      # the diagonal all the same
        found, pi, pj, av, m, d, dm = sh.grm_pairs_raw(0.0, n)      # exactly enough
        assert found == n and np.array_equal(pi[:n], wi) and np.array_equal(pj[:n], wj) and np.array_equal(_bits(av[:n]), _bits(a[wi, wj]))
        got = sh.grm_pairs(0.0, cap=3)                              # the wrapper re-calls once
        assert np.array_equal(got[0], wi) and np.array_equal(got[1], wj) and np.array_equal(_bits(got[2]), _bits(a[wi, wj]))
        found, *_ = sh.grm_pairs_raw(50.0, 0)                       # no pair above the cutoff, no slot
        assert found == 0


def test_kernel_modes_1_and_2_give_identical_bytes():
    cs = gr.case("ragged")
    N = cs["N"]
    res = []
    for mode in (1, 2):
        with _shard(cs, mode=mode) as sh:
            assert sh.get_kernel_mode() == mode
            res.append(sh.grm_weights()[:2] + sh.grm_block(0, N, 0, N) + sh.grm_pairs(0.05))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res[0], res[1]))
    assert len(res[0][4]) > 100


def test_a_grm_call_leaves_the_products_kinship_and_ld_scores_of_the_context_unchanged():
    cs = gr.case("ragged")
    N, M = cs["N"], cs["M"]
    rng = np.random.default_rng(9)
    x = rng.standard_normal(M)
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        sh.compute_markers_statistics()
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)
        before = (sh.Ax(x), sh.ATx(p)) + sh.ld_scores(20) + sh.king_block(5, 100, 300, 50)
        sh.grm_weights()
        sh.grm_block(5, 100, 300, 50)
        sh.grm_pairs(0.1)
        after = (sh.Ax(x), sh.ATx(p)) + sh.ld_scores(20) + sh.king_block(5, 100, 300, 50)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


def test_every_refusal_is_raised_with_its_message():
    cs = gr.case("edge")
    N, M = cs["N"], cs["M"]
    calls = (lambda s: s.grm_block(0, 2, 0, 2), lambda s: s.grm_pairs(0.1), lambda s: s.grm_weights())
    with capi.Shard(N, M, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        for call in calls:
            with pytest.raises(capi.GvError, match="meth"):
                call(sh)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width
        with capi.Shard(N, M, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(N, M, 2, bits).astype(dtype), 1.0 / 127.0)
            for call in calls:
                with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                    call(sh)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(cs["bed"])
        for call in calls:
            with pytest.raises(capi.GvError, match="raw rows alone"):
                call(sh)
    with _shard(cs, layout=1) as sh:              # two stripe sets: the tile layout is the way out
        assert sh.get_layout() == 1
        for call in calls:
            with pytest.raises(capi.GvError, match="two stripe sets.*tile layout"):
                call(sh)
    with _shard(cs) as sh:
        sh.force_multi(1)                         # a job of more than one rank
        for call in calls:
            with pytest.raises(capi.GvError, match="more than one rank"):
                call(sh)
        sh.force_multi(0)
        for i0, ni, j0, nj in ((-1, 2, 0, 2), (0, N + 1, 0, 1), (N, 1, 0, 1), (0, 1, 250, 8), (0, -1, 0, 1), (0, 1, 0, -1)):
            with pytest.raises(capi.GvError, match="outside"):
                sh.grm_block(i0, ni, j0, nj)
        with pytest.raises(capi.GvError, match="cap must not be negative"):
            sh.grm_pairs_raw(0.1, -1)
        for bad in (np.nan, np.inf):
            with pytest.raises(capi.GvError, match="cutoff"):
                sh.grm_pairs(bad)
        L, found = sh.L, capi.C.c_int64(-7)
        d = np.full(N, -3.0)
        assert L.gv_grm_pairs(sh.h, None, 0.1, 4, None, None, None, None, capi._dp(d), None, capi.C.byref(found)) != 0      # NULL arrays, cap > 0
        assert b"NULL" in L.gv_last_error(sh.h) and found.value == -7 and np.all(d == -3.0)                     # nothing written
        assert L.gv_grm_pairs(sh.h, None, 0.1, 0, None, None, None, None, None, None, None) != 0                # NULL n_found
        assert b"n_found is NULL" in L.gv_last_error(sh.h)
        assert L.gv_grm_info(sh.h, None) != 0 and L.gv_grm_block(None, None, 0, 1, 0, 1, None, None) != 0
        a, _ = _whole("edge")
        assert len(sh.grm_pairs(0.1)[0]) == len(gr.pairs(a, 0.1)[0])                                           # and the context still works
