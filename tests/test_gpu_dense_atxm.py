"""The batch ATx kernel of 8-bit dosage codes on the fixed-point route (k_dm_atxm<CP> of gv_dense_atxm.hip behind gv_atxm_dev; DESIGN.md
section 29): every column is BIT-IDENTICAL to gv_atx_dev of that column alone on the same context, and the first and last column of a
batch equal the integer restatement of tests/dosage_fixed_restatement.py bit for bit.

Shapes: dosage_fixed_cases.SHAPES, one per structural edge of k_dm_atx, which the new kernel inherits (under one tile, pitch 192 with
the re-read second half, five 128-row blocks with idle waves and the row clamp, several steps and segments, with and without a
phenotype mask); K-segments: the library's cut, 256 and 64 entries; C in {1, 2, 3, 5, 8, 9, 17}: under a pair, an odd pair, a partial
pass of either width, several passes with a narrow last one.  A restated product is computed once per (case, vector) and shared."""
import numpy as np
import pytest

import dosage_fixed_cases as dc
import test_gpu_dosage as gd
from gvamp_amd import capi
from test_gpu_dosage_fixed import _ref_atx
from test_gpu_dosage_mfma import shard

pytestmark = pytest.mark.gpu
SCALE = dc.SCALE
CS = (1, 2, 3, 5, 8, 9, 17)
# the library's pick (threshold 3, its own columns per pass) and both widths with the kernel forced from one column on
PINS = {"pick": {}, "cols4": dict(GV_ATXM_COLS="4", GV_ATXM_KERNEL="1"), "cols8": dict(GV_ATXM_COLS="8", GV_ATXM_KERNEL="1")}
SETUPS = [(N, M, na, seg, pin) for (N, M, na) in dc.SHAPES for seg in dc.SEGS for pin in PINS]
MIN_COLS = 3          # the threshold of this path (gv_atxm_stats.min_cols)


def _resident(cs, seg=None, route=1, transport=0, **env):
    sh = shard(cs["N"], cs["M"], seg, **env)
    try:
        if transport:
            sh.force_multi(transport)
        sh.set_dosage_route(route)
        sh.upload_dosage(cs["B"], SCALE)
        if cs["with_na"]:
            sh.set_mask(cs["m4"], cs["nonas"])
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (route, route)
        _, msig = sh.marker_stats()
    except BaseException:
        sh.close()
        raise
    return sh, msig


def _pad(sh, p):
    out = np.zeros(4 * sh.mbytes)
    out[:len(p)] = p
    return out


def _column(cs, j):
    """column j of the batches of a case: the four kinds of dosage_fixed_cases in turn (column 0 is the vector the one-vector tests use)"""
    return dc.p_vector(dc.KINDS[j % 4], cs, seed=j // 4)


def _atxm(sh, cols):
    ps, outs = [sh.vecN(_pad(sh, p)) for p in cols], [sh.vecM() for _ in cols]
    try:
        sh.atxm_dev(ps, outs)
        return [o.download() for o in outs]
    finally:
        for v in ps + outs:
            v.free()


def _single(sh, p):
    pv, out = sh.vecN(_pad(sh, p)), sh.vecM()
    try:
        sh.atx_dev(pv, out)
        return out.download()
    finally:
        pv.free()
        out.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _passes(C, cp):
    w = 4 if (C <= 4 or cp == 4) else 8          # gvb::cp_for: a narrow batch takes a narrow instantiation
    return -(-C // w), w


@pytest.mark.parametrize("N,M,with_na,seg,pin", SETUPS)
def test_every_column_is_the_one_vector_product_bit_for_bit(N, M, with_na, seg, pin):
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs, seg, **PINS[pin])
    with sh:
        cols = [_column(cs, j) for j in range(max(CS))]
        want = [_single(sh, p) for p in cols]
        assert any(np.any(w != 0) for w in want) or N == 1
        for C in CS:
            got = _atxm(sh, cols[:C])
            info = sh.atxm_info()
            if pin == "pick" and C < MIN_COLS:
                assert info["path"] == "fallback" and info["passes"] == -(-C // 2), info
            else:
                passes, width = _passes(C, 4 if pin == "cols4" else 8)
                assert info["path"] == "kernel" and info["columns"] == C, info
                assert info["passes"] == passes and info["cols_per_pass"] == width and info["ksegs"] >= 1, info
                assert info["min_cols"] == (MIN_COLS if pin == "pick" else 1) and info["scratch_bytes"] > 0, info
            for j in range(C):
                assert _same_bits(got[j], want[j]), (C, j)
            # the integer restatement at the first and the last column, with the device's msig
            for j in sorted({0, C - 1}):
                ref = _ref_atx(cs, msig, cols[j])
                assert _same_bits(got[j], ref), ("restatement", C, j)


def test_segments_follow_the_cap():
    """GV_DOSAGE_MFMA_SEG = 64 cuts a segment per K-step: ksegs is the step count, and the bits are those of one segment"""
    cs = dc.case(1003, 700, False)
    outs = {}
    for seg in dc.SEGS:
        sh, _ = _resident(cs, seg)
        with sh:
            outs[seg] = _atxm(sh, [_column(cs, j) for j in range(5)])
            info = sh.atxm_info()
            assert info["path"] == "kernel", info
            if seg == 64:
                assert info["ksegs"] == -(-1003 // 128), info
            elif seg == 256:
                assert info["ksegs"] == -(-1003 // 256), info
    for seg in dc.SEGS[1:]:
        assert all(_same_bits(a, b) for a, b in zip(outs[seg], outs[None]))


@pytest.mark.parametrize("N,M,with_na", [(63, 17, False), (130, 70, True), (1003, 700, False)])
def test_special_columns_inside_a_batch(N, M, with_na):
    """zero, NaN, inf, tiny and subnormal columns among ordinary ones: each comes out as gv_atx_dev makes it, and no neighbour moves"""
    cs = dc.case(N, M, with_na)
    sh, _ = _resident(cs)
    with sh:
        cols = []
        for j, kind in enumerate(dc.SPECIAL):
            cols += [_column(cs, j), dc.p_vector(kind, cs)]
        cols.append(_column(cs, 7))
        want = [_single(sh, p) for p in cols]
        got = _atxm(sh, cols)
        assert sh.atxm_info()["path"] == "kernel"
        for j in range(len(cols)):
            assert _same_bits(got[j], want[j]), j
        for j, kind in enumerate(dc.SPECIAL):
            w = got[2 * j + 1]
            if kind == "zero":
                assert not np.any(w)
            elif kind in ("nan", "inf"):
                assert np.all(np.isnan(w))
            else:
                assert np.all(np.isfinite(w)) and np.any(w != 0)
            assert np.all(np.isfinite(got[2 * j]))


def test_order_repetition_and_batch_size_do_not_change_a_column():
    cs = dc.case(200, 513, False)
    sh, _ = _resident(cs)
    with sh:
        cols = [_column(cs, j) for j in range(9)]
        base = _atxm(sh, cols)
        again = _atxm(sh, cols)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
        perm = [8, 3, 0, 5, 1, 7, 2, 6, 4]
        moved = _atxm(sh, [cols[k] for k in perm])
        assert all(_same_bits(moved[i], base[k]) for i, k in enumerate(perm))
        for C in (3, 4, 5, 8):
            assert all(_same_bits(a, b) for a, b in zip(_atxm(sh, cols[:C]), base))
        # the same input handle in several columns
        pv = sh.vecN(_pad(sh, cols[2]))
        outs = [sh.vecM() for _ in range(5)]
        sh.atxm_dev([pv] * 5, outs)
        assert sh.atxm_info()["path"] == "kernel"
        assert all(_same_bits(o.download(), base[2]) for o in outs)
        for v in [pv] + outs:
            v.free()


def test_the_context_is_left_alone():
    """gv_atx_dev, gv_atx2_dev, gv_ax_dev and gv_lmmse_mult give the same bits before and after a batch (the batch has scratch of its own)"""
    cs = dc.case(1003, 700, True)
    sh, msig = _resident(cs)
    with sh:
        x = dc.x_vector("normal", cs, msig)
        p, p2 = _pad(sh, _column(cs, 0)), _pad(sh, _column(cs, 1))

        def products():
            xv, zv, lm = sh.vecM(x), sh.vecN(), sh.vecM()
            sh.ax_dev(xv, zv)
            sh.lmmse_mult(xv, dc.TAU, dc.GAM2, lm)
            pa, pb, wa, wb = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
            sh.atx2_dev(pa, pb, wa, wb)
            res = [_single(sh, p[:cs["N"]]), zv.download(), lm.download(), wa.download(), wb.download()]
            for v in (xv, zv, lm, pa, pb, wa, wb):
                v.free()
            return res

        before = products()
        _atxm(sh, [_column(cs, j) for j in range(9)])
        assert sh.atxm_info()["path"] == "kernel"
        after = products()
        assert all(_same_bits(a, b) for a, b in zip(before, after))
        assert all(np.any(a != 0) for a in before)


@pytest.mark.parametrize("what", ["route0", "dosage16", "reserved", "na-kernels", "kernel-off", "forced-multi"])
def test_other_paths_report_themselves_and_keep_the_bits(what):
    """the kernel needs route 1 in force: 8-bit codes and the plain kernels.  Everything else is the fallback in ceil(C / 2) passes;
    gv_debug_force_multi keeps the kernel (ATx issues no collective)"""
    N, M = 515, 300
    env = {"na-kernels": dict(GV_DOSAGE_NA_KERNELS="1"), "kernel-off": dict(GV_ATXM_KERNEL="0")}.get(what, {})
    sh = shard(N, M, None, **env)
    with sh:
        if what == "forced-multi":
            sh.force_multi(1)
        if what in ("reserved", "na-kernels"):
            sh.set_dosage_missing(1)
        sh.set_dosage_route(0 if what == "route0" else 1)
        if what == "reserved":
            sh.synth_dosage_na(3, 8, 50000)
        else:
            sh.synth_dosage(3, 16 if what == "dosage16" else 8)
        m4, _, nonas = gd.na_mask(N, False)
        sh.set_mask(m4, nonas)
        sh.compute_markers_statistics()
        in_force = sh.dosage_route()[1]
        assert in_force == (1 if what in ("kernel-off", "forced-multi") else 0), (what, sh.dosage_route())
        rng = np.random.default_rng(9)
        cols = [rng.standard_normal(N) * 10.0 ** k for k in range(5)]
        want = [_single(sh, p) for p in cols]
        for C in (1, 2, 5):
            got = _atxm(sh, cols[:C])
            info = sh.atxm_info()
            if what == "forced-multi" and C >= MIN_COLS:
                assert info["path"] == "kernel" and info["columns"] == C and info["ksegs"] >= 1, info
            else:
                assert info["path"] == "fallback" and info["columns"] == C and info["ksegs"] == 0, info
                assert info["passes"] == -(-C // 2), info
            assert all(_same_bits(got[j], want[j]) for j in range(C)), (what, C)
        assert any(np.any(w != 0) for w in want)


def test_gv_create_refuses_a_bad_tile_count(monkeypatch):
    monkeypatch.setenv("GV_ATXM_TILES", "6")
    with pytest.raises(capi.GvError, match="4 or 8"):
        capi.Shard(16, 64)


@pytest.mark.parametrize("tiles", ["4", "8"])
def test_either_tile_count_gives_the_same_bits(tiles):
    cs = dc.case(200, 513, False)
    sh, _ = _resident(cs, None, GV_ATXM_TILES=tiles)
    with sh:
        cols = [_column(cs, j) for j in range(9)]
        want = [_single(sh, p) for p in cols]
        for C in (3, 9):
            got = _atxm(sh, cols[:C])
            assert sh.atxm_info()["path"] == "kernel"
            assert all(_same_bits(got[j], want[j]) for j in range(C)), (tiles, C)
