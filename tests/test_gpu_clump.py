"""LD clumping on the GPU (gv_ld_clump) against the numpy restatement of tests/clump_restatement.py: both layouts
and both MFMA kernel modes, uniform / clustered / tied positions, chromosomes, three thresholds, a threshold set exactly on a pair's own
r^2, a deep chain of dependencies, the order and eligibility rules, the filtered launch, reproducibility, the rest of the context left as
it was, the refusals and the driver.

index_of and n_index are exact.  Where the threshold is not taken from the device's own bits, the test first asserts that no in-band
pair of the restatement lies within 1e-9 of it: the device's r is within 1e-12 of the restatement's (section 16), so no comparison can
fall the other way."""
import math
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth
import clump_restatement as cr
import ld_pos_restatement as lpr
import ld_restatement as ldr
import precond_restatement as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = ((2, 1), (1, 1), (2, 2), (1, 2))          # (resident layout: 1 two stripe sets, 2 the tile layout; kernel mode)
N, S = 333, 37                                     # no multiple of 256 or 128: a masked tail; a few individuals without a phenotype
MARGIN = 1e-9


def _mask4(na):
    m = np.zeros((na.size + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(bed, n, M, s=0, layout=2, mode=1, na=None, stats=True):
    sh = capi.Shard(n, M, Mt=s + M + 100, S=s, device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(bed)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    if stats:
        sh.compute_markers_statistics()
    return sh


def _restate(g, na):
    bed = ldr.encode(g)
    a, b = pr.decode(bed, g.shape[0], g.shape[1])
    mave, msig = pr.marker_stats(a, b, na)
    r, poly = ldr.corr(ldr.gram(a, b, na, mave, msig))
    return dict(bed=bed, na=na, r=r, poly=poly)


_DATA = {}


def _data(M):
    """genotypes with LD blocks and missing entries, hand-placed markers, the mask, and r / poly of the restatement -- once per M.
    M = "chain": 300 markers of a thresholded AR(1) sequence, LD from neighbour to neighbour"""
    if M not in _DATA:
        na = np.ones(N)
        na[::13] = 0.0
        if M == "chain":
            rng = np.random.default_rng(1)
            z = np.empty((2, N, 300))
            z[:, :, 0] = rng.standard_normal((2, N))
            for j in range(1, 300):
                z[:, :, j] = 0.95 * z[:, :, j - 1] + math.sqrt(1 - 0.95 ** 2) * rng.standard_normal((2, N))
            g = (z[0] > 0).astype(np.int64) + (z[1] > 0)
            g[rng.random(g.shape) < 0.02] = -1
        else:
            a, b = pr.decode(synth.synth_bed(N, M, seed=5, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000), N, M)
            g = np.where(b > 0, a, -1).astype(np.int64)
            g[:, 10] = 0                         # all zero
            g[:, 20] = -1                        # missing everywhere
            g[:, 31] = g[:, 30]                  # equal to its neighbour
            if M > 63:
                g[:, 63] = g[:, 5]               # a copy across the row-group edge ...
                g[::17, 63] = -1                 # ... partly missing
        d = _restate(g, na)
        if M != "chain":
            assert list(np.nonzero(~d["poly"])[0]) == [10, 20] and abs(d["r"][30, 31] - 1) < 1e-12
        _DATA[M] = d
    return _DATA[M]


@pytest.fixture(scope="module")
def shards():
    """one context per (M, layout, kernel mode), opened on first use and closed with the module"""
    held = {}

    def get(M, layout=2, mode=1):
        if (M, layout, mode) not in held:
            d = _data(M)
            held[(M, layout, mode)] = _shard(d["bed"], N, 300 if M == "chain" else M, s=S, layout=layout, mode=mode, na=d["na"])
            assert held[(M, layout, mode)].get_layout() == layout
        return held[(M, layout, mode)]

    yield get
    for sh in held.values():
        sh.close()


def _positions(M):
    """name -> (pos, chrom or None, radius)"""
    j = np.arange(M)
    out = {"arange, radius 70": (S + j * 1.0, None, 70.0)}
    if M == 300:
        # 0..39 alone (10 apart), 40..63 three to a radius, 64..279 two hundred to a radius, 280..299 alone again
        gaps = np.where(j < 40, 10.0, np.where(j < 64, 0.3, np.where(j < 280, 0.005, 10.0)))
        gaps[40] = gaps[64] = gaps[280] = 10.0
    else:
        gaps = np.where(j < 20, 10.0, 0.02)
    out["clustered"] = (np.cumsum(gaps), None, 1.0)
    ties2 = ((j + 3) // 7) * 1.0              # 60..66 is one run straddling 63 / 64
    out["ties straddling 63 / 64"] = (ties2, None, 2.0)
    if M == 300:
        walk = np.cumsum(np.random.default_rng(8).exponential(1.0, M))
        ch3 = np.repeat([2, 9, 4], [64, M - 65, 1])
        out["three chromosomes, breaks at 64 and M - 1"] = (walk, ch3, 90.0)
    return out


def _want(d, pos, radius, chrom, p, p1, p2, r2, check_margin=True):
    if check_margin:          # a condition on the inputs, not a measurement
        assert cr.margin(d["r"], lpr.in_band_pos(pos, radius, chrom), r2) >= MARGIN, (radius, r2)
    adj = cr.adjacency(d["r"], d["poly"], pos, radius, chrom, p, p2, r2)
    return cr.clump_sequential(adj, p, p1, p2)


def _same(got, want):
    return got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("M", [300, 130, 40])
def test_clumps_match_the_sequential_definition_on_both_layouts_and_modes(shards, M):
    d = _data(M)
    p = np.random.default_rng(M).random(M) * 0.02
    p1, p2 = 0.01, 0.02
    e1, e2 = cr.eligible(p, p1, p2)
    assert e2.all() and 0 < e1.sum() < M
    for pname, (pos, chrom, radius) in _positions(M).items():
        hi = lpr.window_hi(pos, radius, chrom)
        for r2 in (0.2, 0.5, 0.8):
            want = _want(d, pos, radius, chrom, p, p1, p2, r2)
            outs = []
            for layout, mode in COMBOS:
                sh = shards(M, layout, mode)
                got = sh.ld_clump(pos, radius, p, p1, p2, r2, chrom=chrom)
                assert _same(got, want), (pname, r2, layout, mode, np.nonzero(got[0] != want[0])[0][:10])
                outs.append(got)
                if (layout, mode) == COMBOS[0]:
                    info, last = sh.ld_info(), sh.ld_clump_last()
                    assert info["block_pairs"] == cr.blocks_launched(hi, e2) == lpr.block_pairs(hi), (pname, info)
                    assert info["useful_macs"] == 4.0 * N * cr.pairs_e2(pos, radius, chrom, e2) == 4.0 * N * lpr.entries(pos, radius, chrom)
                    assert info["seconds"] > 0 and info["scratch_bytes"] >= 8 * 64 * (2 * lpr.dmax_of(hi) + 1) * ((M + 63) // 64)
                    assert last["n_e1"] == e1.sum() and last["n_e2"] == M and 1 <= last["rounds"] <= e1.sum()
                    assert sh.ld_last_passes() == 1
                    assert _same(sh.ld_clump(pos, radius, p, p1, p2, r2, chrom=chrom), got)          # two calls
            for o in outs[1:]:               # layouts and kernel modes agree
                assert _same(o, outs[0]), (pname, r2)
        # the copy of the neighbour and the partly missing copy across 63 / 64 are what the thresholds see them as
        if pname == "arange, radius 70":
            want = _want(d, pos, radius, chrom, np.zeros(M), 1.0, 1.0, 0.8)
            assert want[0][31] == 30 and (M < 64 or want[0][63] == 5) and want[0][10] == 10 and want[0][20] == 20


def test_a_threshold_exactly_on_a_pairs_own_bits(shards):
    """r2 = r_jk * r_jk of the device's own gv_ld_band bits: both sides threshold the same bits, so no margin is needed and the chosen
    pair must come out adjacent"""
    M, B = 300, 70
    d = _data(M)
    pos = S + np.arange(M) * 1.0
    p = np.random.default_rng(3).random(M) * 0.02
    for layout, mode in COMBOS:
        sh = shards(M, layout, mode)
        band = sh.ld_band(B, 0, M)
        r = np.zeros((M, M))
        for dd in range(-B, B + 1):
            j = np.arange(max(0, -dd), min(M, M - dd))
            r[j, j + dd] = band[j, B + dd]
        assert np.array_equal(r, r.T) and np.abs(r - np.where(lpr.in_band_pos(pos, 70.0), d["r"], 0.0)).max() < 1e-12
        x = r * r
        # pairs across the row-group edge 63 / 64, inside a row group, and two row groups apart
        cands = [(j, k) for j, k in ((60, 66), (62, 64), (5, 63), (63, 69), (100, 103), (250, 256), (120, 190), (30, 31))
                 if 0.02 < x[j, k] <= 1.0]
        assert len(cands) >= 4
        for j, k in cands:
            r2 = float(r[j, k] * r[j, k])
            adj = lpr.in_band_pos(pos, 70.0) & ~np.eye(M, dtype=bool) & d["poly"][:, None] & d["poly"][None, :] & (x >= r2)
            assert adj[j, k] and adj[k, j]
            for p1, p2 in ((0.01, 0.02), (1.0, 1.0)):
                pp = p if p1 < 1.0 else np.where(np.arange(M) == j, 0.0, 0.5 + p)          # (j leads: k must be its member, or an earlier clump's)
                want = cr.clump_sequential(adj, pp, p1, p2)
                got = sh.ld_clump(pos, 70.0, pp, p1, p2, r2)
                assert _same(got, want), (layout, mode, j, k, r2)
                if p1 == 1.0:
                    assert got[0][j] == j and got[0][k] == j
            # one ulp above the pair's own value the pair is no longer adjacent
            up = math.nextafter(r2, 2.0)
            if up <= 1.0:
                adj_up = adj & (x >= up)
                assert not adj_up[j, k]
                pp = np.where(np.arange(M) == j, 0.0, 0.5 + p)
                assert _same(sh.ld_clump(pos, 70.0, pp, 1.0, 1.0, up), cr.clump_sequential(adj_up, pp, 1.0, 1.0))


def test_a_deep_chain_of_dependencies(shards):
    """LD from neighbour to neighbour and p increasing along the markers: every marker waits for the one before it"""
    M = 300
    d = _data("chain")
    pos = S + np.arange(M) * 1.0
    p = np.arange(M) / (2.0 * M)
    r2 = 0.5
    assert cr.margin(d["r"], lpr.in_band_pos(pos, 70.0), r2) >= MARGIN
    adj = cr.adjacency(d["r"], d["poly"], pos, 70.0, None, p, 1.0, r2)
    want = cr.clump_sequential(adj, p, 1.0, 1.0)
    by_rounds = cr.clump_rounds(adj, p, 1.0, 1.0)
    print("rounds of the synchronous scheme:", by_rounds[2])
    assert by_rounds[2] >= 50 and _same(by_rounds[:2], want)
    for layout, mode in COMBOS:
        sh = shards("chain", layout, mode)
        got = sh.ld_clump(pos, 70.0, p, 1.0, 1.0, r2)
        assert _same(got, want), (layout, mode)
        last = sh.ld_clump_last()
        assert 2 <= last["rounds"] <= M and last["n_e1"] == last["n_e2"] == M
    # the reverse order and an order of random ties
    for pp in (p[::-1].copy(), np.random.default_rng(4).integers(0, 3, M) * 0.1):
        adj = cr.adjacency(d["r"], d["poly"], pos, 70.0, None, pp, 1.0, r2)
        assert _same(shards("chain").ld_clump(pos, 70.0, pp, 1.0, 1.0, r2), cr.clump_sequential(adj, pp, 1.0, 1.0))


def test_order_and_eligibility(shards):
    M = 300
    d = _data(M)
    sh = shards(M)
    pos, radius, r2 = S + np.arange(M) * 1.0, 70.0, 0.5
    assert cr.margin(d["r"], lpr.in_band_pos(pos, radius), r2) >= MARGIN
    full = cr.adjacency(d["r"], d["poly"], pos, radius, None, np.zeros(M), 1.0, r2)
    assert full[30, 31] and full[5, 63]
    # equal p: the lower index wins
    got = sh.ld_clump(pos, radius, np.zeros(M), 0.0, 0.0, r2)
    assert _same(got, cr.clump_sequential(full, np.zeros(M), 0.0, 0.0))
    assert (got[0] >= 0).all() and (got[0] <= np.arange(M)).all() and got[0][0] == 0          # an index marker is the first of its clump
    p = np.full(M, 0.5)
    p[31] = p[30] = 0.001
    got = sh.ld_clump(pos, radius, p, 0.01, 1.0, r2)
    assert got[0][30] == 30 and got[0][31] == 30 and _same(got, _want(d, pos, radius, None, p, 0.01, 1.0, r2))
    p[31], p[30] = 0.001, 0.002          # the higher index with the lower p leads
    got = sh.ld_clump(pos, radius, p, 0.01, 1.0, r2)
    assert got[0][31] == 31 and got[0][30] == 31 and _same(got, _want(d, pos, radius, None, p, 0.01, 1.0, r2))
    # p in (p1, p2]: never an index; -1 when no index reaches it.  NaN or p > p2: -1 and never claimed
    p = np.full(M, 0.015)                # members only ...
    p[30] = 0.001                        # ... but one index
    p[31] = math.nan
    nb = np.nonzero(full[30])[0]
    assert nb.size >= 2 and 31 in nb
    p[nb[nb != 31][0]] = 0.03            # a neighbour above p2
    got = sh.ld_clump(pos, radius, p, 0.01, 0.02, r2)
    want = _want(d, pos, radius, None, p, 0.01, 0.02, r2)
    assert _same(got, want) and got[1] == 1 and got[0][30] == 30 and got[0][31] == -1 and got[0][nb[nb != 31][0]] == -1
    claimed = np.nonzero(got[0] == 30)[0]
    assert set(claimed) == {30} | (set(nb) - {31, nb[nb != 31][0]}) and (np.delete(got[0], claimed) == -1).all()
    last = sh.ld_clump_last()
    assert last["n_e1"] == 1 and last["n_e2"] == M - 2 and last["rounds"] == 1
    # E1 empty: all -1, no index, no round
    for p1, pv in ((0.0, p), (0.01, np.full(M, math.nan)), (0.01, np.full(M, 0.015))):
        got = sh.ld_clump(pos, radius, pv, p1, 0.02, r2)
        assert (got[0] == -1).all() and got[1] == 0 and sh.ld_clump_last()["rounds"] == 0 and sh.ld_clump_last()["n_e1"] == 0
    # a monomorphic marker in E1 is a clump of one, whatever its neighbours
    p = np.full(M, 0.5)
    p[[10, 20]] = 0.001
    p[[9, 11, 19, 21]] = 0.015
    got = sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.0)
    assert got[1] == 2 and got[0][10] == 10 and got[0][20] == 20 and (np.delete(got[0], [10, 20]) == -1).all()
    # r2 = 0 joins every polymorphic pair of the band (r * r >= 0 holds whatever the last bits of r are)
    p = np.random.default_rng(6).random(M) * 0.02
    adj = cr.adjacency(d["r"], d["poly"], pos, radius, None, p, 0.02, 0.0)
    assert _same(sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.0), cr.clump_sequential(adj, p, 0.01, 0.02))


def test_only_the_blocks_with_eligible_markers_are_launched(shards):
    M = 300
    d = _data(M)
    rng = np.random.default_rng(7)
    p = np.ones(M)
    p[:64] = rng.random(64) * 0.02
    p[192:256] = rng.random(64) * 0.02
    e1, e2 = cr.eligible(p, 0.01, 0.02)
    assert set(np.nonzero(e2)[0] // 64) == {0, 3}
    for radius, launched in ((70.0, 2), (200.0, 3)):          # (0, 0) and (3, 3); with the longer reach (0, 3) too
        pos = S + np.arange(M) * 1.0
        hi = lpr.window_hi(pos, radius)
        assert cr.blocks_launched(hi, e2) == launched < lpr.block_pairs(hi)
        want = _want(d, pos, radius, None, p, 0.01, 0.02, 0.2)
        for layout, mode in COMBOS:
            sh = shards(M, layout, mode)
            assert _same(sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.2), want), (radius, layout, mode)
            info = sh.ld_info()
            assert info["block_pairs"] == launched
            assert info["useful_macs"] == 4.0 * N * cr.pairs_e2(pos, radius, None, e2)
    assert (want[0][64:192] == -1).all() and (want[0][256:] == -1).all()
    # nothing eligible: nothing launched
    sh = shards(M)
    got = sh.ld_clump(pos, 70.0, np.ones(M), 0.01, 0.02, 0.2)
    assert (got[0] == -1).all() and got[1] == 0 and sh.ld_info()["block_pairs"] == 0 and sh.ld_info()["useful_macs"] == 0.0


def test_the_context_is_left_as_it_was():
    M = 300
    d = _data(M)
    x = np.random.default_rng(1).standard_normal(M)
    pos, chrom, radius = _positions(M)["clustered"]
    p = np.random.default_rng(2).random(M) * 0.02
    for layout, mode in ((1, 1), (2, 2)):
        with _shard(d["bed"], N, M, s=S, layout=layout, mode=mode, na=d["na"]) as sh:
            sh.set_cg_precond("ld", 64)
            z = sh.Ax(x)
            w = sh.ATx(z)
            l2 = sh.ld_scores_pos(pos, radius, adjusted=True)
            gram = [sh.precond_window_gram(0, 1), sh.precond_window_gram(1, 2)]
            first = sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.5)
            sh.ld_clump(S + np.arange(M) * 1.0, 100.0, p, 0.02, 0.02, 0.2)
            assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(z), w)
            again = sh.ld_scores_pos(pos, radius, adjusted=True)
            assert np.array_equal(again[0], l2[0], equal_nan=True) and np.array_equal(again[1], l2[1])
            assert all(np.array_equal(a, b) for a, b in zip(gram, [sh.precond_window_gram(0, 1), sh.precond_window_gram(1, 2)]))
            assert _same(sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.5), first)


def test_refusals(shards):
    M = 300
    d = _data(M)
    pos = np.arange(M) * 1.0
    p = np.full(M, 0.001)
    n2, M2 = 600, 256
    with capi.Shard(n2, M2, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="gv_ld_clump.*meth"):
            sh.ld_clump(np.arange(M2) * 1.0, 3.0, np.zeros(M2), 0.01, 0.02, 0.5)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width, with and without gv_set_ld_dosage
        with capi.Shard(n2, M2, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(n2, M2, 2, bits).astype(dtype), 1.0 / 127.0)
            sh.set_mask(_mask4(np.ones(n2)), n2)
            sh.compute_markers_statistics()
            for on in (0, 1):
                sh.set_ld_dosage(on)
                with pytest.raises(capi.GvError, match=r"gv_ld_clump: bed data only.*%d-bit codes.*gv_set_ld_dosage" % bits):
                    sh.ld_clump(np.arange(M2) * 1.0, 3.0, np.zeros(M2), 0.01, 0.02, 0.5)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(d["bed"])
        sh.set_kernel_mode(0)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="gv_ld_clump.*re-encoded"):
            sh.ld_clump(pos, 3.0, p, 0.01, 0.02, 0.5)
    with _shard(d["bed"], N, M, stats=False) as sh:    # statistics not computed
        with pytest.raises(capi.GvError, match="gv_ld_clump: marker statistics must be computed first"):
            sh.ld_clump(pos, 3.0, p, 0.01, 0.02, 0.5)
    sh = shards(M)
    with pytest.raises(capi.GvError, match="gv_ld_clump: pos is NULL"):
        sh.ld_clump(None, 3.0, p, 0.01, 0.02, 0.5)
    with pytest.raises(capi.GvError, match="gv_ld_clump: p is NULL"):
        sh.ld_clump(pos, 3.0, None, 0.01, 0.02, 0.5)
    out = np.zeros(M, dtype=np.int64)
    C = capi.C
    args = (sh.h, pos.ctypes.data_as(C.POINTER(C.c_double)), 3.0, None, p.ctypes.data_as(C.POINTER(C.c_double)), 0.01, 0.02, 0.5)
    assert sh.L.gv_ld_clump(*args, None, None) != 0 and b"gv_ld_clump: index_of is NULL" in sh.L.gv_last_error(sh.h)
    assert sh.L.gv_ld_clump(*args, out.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0          # (n_index may be NULL)
    assert np.array_equal(out, sh.ld_clump(pos, 3.0, p, 0.01, 0.02, 0.5)[0])
    for radius in (-1.0, math.nan, math.inf):
        with pytest.raises(capi.GvError, match="gv_ld_clump: radius must be finite and >= 0"):
            sh.ld_clump(pos, radius, p, 0.01, 0.02, 0.5)
    for p1, p2, r2, msg in ((math.nan, 0.02, 0.5, "p1 and p2 must be finite"), (0.01, math.inf, 0.5, "p1 and p2 must be finite"),
                            (0.01, 0.02, math.nan, "r2 must be finite"), (0.03, 0.02, 0.5, "p1 must not exceed p2"),
                            (-0.01, 0.02, 0.5, "p1 must be >= 0"), (-0.02, -0.01, 0.5, "p1 must be >= 0"),
                            (0.01, 0.02, -0.1, r"r2 must be in \[0, 1\]"), (0.01, 0.02, 1.5, r"r2 must be in \[0, 1\]")):
        with pytest.raises(capi.GvError, match="gv_ld_clump: " + msg):
            sh.ld_clump(pos, 3.0, p, p1, p2, r2)
    bad = pos.copy()
    bad[5] = math.nan
    with pytest.raises(capi.GvError, match=r"gv_ld_clump: pos\[5\] is not finite"):
        sh.ld_clump(bad, 3.0, p, 0.01, 0.02, 0.5)
    bad = pos.copy()
    bad[77] = 75.5
    with pytest.raises(capi.GvError, match=r"gv_ld_clump: pos\[77\] = 75.5 is below pos\[76\] = 76 .*must not decrease"):
        sh.ld_clump(bad, 3.0, p, 0.01, 0.02, 0.5)
    with pytest.raises(capi.GvError, match="gv_ld_clump: chromosome id 1 reappears at marker 100"):
        sh.ld_clump(pos, 3.0, p, 0.01, 0.02, 0.5, chrom=np.repeat([1, 2, 1], [50, 50, 200]))
    n, Mb = 40, 8194                         # a reach above 8192
    with _shard(synth.synth_bed(n, Mb, seed=2, miss_ppm=20000), n, Mb) as sh2:
        with pytest.raises(capi.GvError, match=r"gv_ld_clump: marker 0 reaches 8193 markers ahead"):
            sh2.ld_clump(np.zeros(Mb), 0.0, np.ones(Mb), 0.01, 0.02, 0.5)
    with capi.Shard(100, 0, Mt=10, S=10, device=0) as sh0:          # M == 0 returns 0 and touches nothing
        sh0.set_layout(False, 2)
        sh0.upload_bed(np.zeros(0, dtype=np.uint8))
        sh0.compute_markers_statistics()
        e, nidx = np.zeros(1), C.c_int64(7)
        out[:] = 7
        dp = C.POINTER(C.c_double)
        rc = sh0.L.gv_ld_clump(sh0.h, e.ctypes.data_as(dp), 3.0, None, e.ctypes.data_as(dp), 0.01, 0.02, 0.5,
                               out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nidx))
        assert rc == 0, sh0.L.gv_last_error(sh0.h)
        assert (out == 7).all() and nidx.value == 7


def test_driver_clumps_a_p_file(tmp_path):
    n, Mt = 203, 150
    a, b = pr.decode(synth.synth_bed(n, Mt, seed=3, miss_ppm=20000, ld_block=48, ld_ppm=900000), n, Mt)
    g = np.where(b > 0, a, -1).astype(np.int64)
    g[:, 12] = 2                              # monomorphic
    bed = ldr.encode(g)
    bfile, pfile, bim, pvals = (str(tmp_path / f) for f in ("g.bed", "y.phen", "g.bim", "g_assoc_p.bin"))
    synth.write_bed(bfile, bed)
    rng = np.random.default_rng(6)
    j = np.arange(Mt)
    chrom = np.where(j < 90, 1, 2).astype(np.int32)
    bp = np.cumsum(rng.integers(1, 4000, Mt))
    bp = np.where(j < 90, bp, bp - bp[90] + 500)
    cm = bp * 1.3e-4
    with open(bim, "w") as f:
        for i in range(Mt):
            f.write("%d\trs%d\t%s\t%d\tA\tG\n" % (chrom[i], i, repr(float(cm[i])), bp[i]))
    na = np.ones(n)
    na[::11] = 0.0
    y = rng.standard_normal(n)
    with open(pfile, "w") as f:
        for i in range(n):
            f.write("F%d I%d %s\n" % (i, i, repr(float(y[i])) if na[i] else "NA"))
    p = rng.random(Mt) * 0.02
    p[12] = 1e-5
    p[40] = math.nan
    p.tofile(pvals)
    d = _restate(g, na)
    assert not d["poly"][12]
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    out = str(tmp_path / "out") + "/"
    base = [exe, "--run-mode", "clump", "--bed-file", bfile, "--phen-files", pfile, "--N", str(n), "--Mt", str(Mt), "--out-dir", out,
            "--out-name", "g"]
    thr = ["--clump-p1", "0.005", "--clump-p2", "0.015", "--clump-r2", "0.2"]
    for flags, pos, radius, label in ((["--bim-file", bim, "--clump-kb", "20"], bp * 1.0, 20000.0, "20 kb"),
                                      (["--bim-file", bim, "--ld-wind-cm", "2.5"], cm, 2.5, "2.5 cM"),
                                      (["--bim-file", bim, "--ld-window", "30"], j * 1.0, 30.0, "30")):
        res = subprocess.run(base + flags + ["--clump-p-file", pvals] + thr, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        want = _want(d, pos, radius, chrom, p, 0.005, 0.015, 0.2)
        got = np.fromfile(out + "g_clump_index.bin")
        assert np.array_equal(got, want[0].astype(np.float64)), label
        with open(out + "g_clumps.txt") as f:
            lines = [ln.split() for ln in f.read().splitlines()]
        assert len(lines) == want[1] and lines[0][0] == "rs12" and lines[0][4] == "0"
        lead = [int(ln[0][2:]) for ln in lines]
        assert lead == list(cr.order_of(p, want[0] == np.arange(Mt)))
        for ln in lines:
            i = int(ln[0][2:])
            members = [int(x[2:]) for x in ln[5].split(",")] if len(ln) > 5 else []
            assert int(ln[1]) == chrom[i] and float(ln[2]) == pos[i] and float(ln[3]) == p[i] and int(ln[4]) == len(members)
            assert members == [k for k in np.nonzero(want[0] == i)[0] if k != i]
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("LD clumping: window " + label)]
        assert len(line) == 1 and "%d clumps" % want[1] in line[0] and "rounds" in line[0] and "blocks launched" in line[0]
        os.remove(out + "g_clump_index.bin")
        os.remove(out + "g_clumps.txt")
    # the default window is 250 kb
    res = subprocess.run(base + ["--bim-file", bim, "--clump-p-file", pvals], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "LD clumping: window 250 kb, p1 0.0001, p2 0.01, r2 0.5" in res.stdout
    assert np.array_equal(np.fromfile(out + "g_clump_index.bin"), _want(d, bp * 1.0, 250000.0, chrom, p, 1e-4, 1e-2, 0.5)[0].astype(np.float64))
    os.remove(out + "g_clump_index.bin")
    # the FATAL lines
    short = str(tmp_path / "short.bin")
    p[:-3].tofile(short)
    for flags, env, msg in ((["--bim-file", bim, "--clump-p-file", short], {}, "holds 1176 bytes, fewer than the 1200"),
                            (["--bim-file", bim, "--clump-p-file", str(tmp_path / "none.bin")], {}, "FATAL: cannot open the p file"),
                            (["--bim-file", bim], {}, "FATAL: --run-mode clump needs --clump-p-file"),
                            (["--clump-p-file", pvals], {}, "FATAL: --clump-kb needs --bim-file"),
                            (["--bim-file", bim, "--clump-p-file", pvals, "--clump-kb", "20", "--ld-window", "50"], {},
                             "FATAL: exactly one of --clump-kb, --ld-wind-cm and --ld-window"),
                            (["--bim-file", bim, "--clump-p-file", pvals], {"WORLD_SIZE": "2", "RANK": "0"}, "runs on one rank"),
                            (["--bim-file", bim, "--clump-p-file", pvals, "--geno-format", "dosage8"], {}, "2-bit genotypes only"),
                            (["--bim-file", bim, "--clump-p-file", pvals, "--clump-p1", "0.5"], {}, "p1 must not exceed p2")):
        res = subprocess.run(base + flags, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert res.returncode != 0 and msg in res.stdout + res.stderr, (flags, res.stdout[-2000:])
        assert not os.path.exists(out + "g_clump_index.bin")
