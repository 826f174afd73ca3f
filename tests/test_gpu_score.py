"""gv_score_dev / gv_score: Z = A W, many weight vectors in one pass over the resident genotypes.

The promise is bit identity: column j equals gv_ax_dev of that column alone -- on the kernel path (tile layout, kernel mode 1, one
rank) under the library's pick and under the development overrides GV_SCORE_COLS / GV_SCORE_KS, and on the fallback everywhere else.
Columns 0 and C - 1 of a batch are also held to the integer restatement of tests/bed_fixed_restatement.py, something outside the
kernels.  Inputs: the two shapes of that module (ragged: N = 1003 x M = 517, last row group and last K-step ragged, NA phenotypes, a
monomorphic and an all-missing marker; even: N = 2100 x M = 1100) and its four kinds of vector (different exponents, the quantiser's
tie and flush probes, a zero vector)."""
import numpy as np
import pytest

import bed_fixed_restatement as bx
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
COUNTS = (1, 2, 3, 5, 8, 16, 17, 33)
PINS = [dict()] + [dict(GV_SCORE_COLS=str(cp), GV_SCORE_KS=str(ks)) for cp in (4, 16) for ks in (1, 3)]
_CACHE = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GV_SCORE_COLS", "GV_SCORE_KS", "GV_SCORE_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = bx.case(name)
    return _CACHE[name]


def _shard(cs, layout=2, mode=1, env=None, kernel="1"):
    """kernel: GV_SCORE_KERNEL of the context ("1": the kernel from one column on, None: the library's threshold)"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        if kernel is not None:
            mp.setenv("GV_SCORE_KERNEL", kernel)
        sh = capi.Shard(cs["N"], cs["M"])
    if layout == "raw":
        sh.set_layout(True, 1)
    else:
        sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(cs["bed"])
    if cs["m4"] is not None:
        sh.set_mask(cs["m4"], cs["nonas"])
    sh.compute_markers_statistics()
    return sh


def _columns(cs, sh, C):
    mave, msig = sh.marker_stats()
    kinds = [bx.vector_x(cs, k, 1, mave, msig) for k in (1, 2, 3, 4)]
    return [kinds[j % 4] for j in range(C)]


def _singles(sh, cols):
    """gv_ax_dev of every column alone"""
    out = []
    xv, zv = sh.vecM(), sh.vecN()
    for x in cols:
        xv.upload(x)
        sh.ax_dev(xv, zv)
        out.append(zv.download())
    xv.free()
    zv.free()
    return out


def _score(sh, cols):
    xs, zs = [sh.vecM(x) for x in cols], [sh.vecN().fill(7.0) for _ in cols]
    sh.score_dev(xs, zs)
    out = [z.download() for z in zs]
    for v in xs + zs:
        v.free()
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. bit identity to the one-vector product ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pin", PINS, ids=lambda p: "pick" if not p else "cols%s-ks%s" % (p["GV_SCORE_COLS"], p["GV_SCORE_KS"]))
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_every_column_equals_the_one_vector_product(name, pin):
    cs = _case(name)
    with _shard(cs, env=pin) as sh:
        assert sh.get_layout() == 2 and sh.get_kernel_mode() == 1
        cols = _columns(cs, sh, max(COUNTS))
        want = _singles(sh, cols)
        pres = np.zeros(len(want[0]), dtype=bool)
        pres[:cs["N"]] = True if cs["present"] is None else cs["present"]
        for C in COUNTS:
            got = _score(sh, cols[:C])
            info = sh.score_info()
            cp = info["cols_per_pass"]
            assert info["path"] == "kernel" and info["columns"] == C and info["passes"] == -(-C // cp), info
            if pin:
                assert cp <= int(pin["GV_SCORE_COLS"]) and info["ksegs"] == int(pin["GV_SCORE_KS"]), info
                assert cp == int(pin["GV_SCORE_COLS"]) or C <= cp      # a narrow batch may take a narrower instantiation
            for j in range(C):
                bad = np.nonzero(got[j].view(np.uint64) != want[j].view(np.uint64))[0]
                assert len(bad) == 0, (C, j, bad[:5], got[j][bad[:5]], want[j][bad[:5]])
                assert np.all(got[j][~pres] == 0.0)                    # pads and NA rows: exact zeros (the outputs were filled with 7)
                assert np.any(got[j] != 0) == (j % 4 != 3)             # kind 4 is the zero vector


def test_the_library_pick_takes_the_kernel_from_min_cols_on():
    cs = _case("ragged")
    with _shard(cs, kernel=None) as sh:
        cols = _columns(cs, sh, 17)
        want = _singles(sh, cols)
        for C in COUNTS[:-1]:
            got = _score(sh, cols[:C])
            info = sh.score_info()
            assert info["min_cols"] >= 1
            assert info["path"] == ("kernel" if C >= info["min_cols"] else "fallback"), info
            assert all(_same_bits(got[j], want[j]) for j in range(C)), (C, info)


def test_host_entry_point_and_repeated_inputs():
    cs = _case("ragged")
    with _shard(cs) as sh:
        cols = _columns(cs, sh, 5)
        want = _singles(sh, cols)
        Z = sh.score(np.array(cols))
        assert Z.shape == (5, 4 * sh.mbytes) and sh.score_info()["path"] == "kernel" and sh.score_info()["seconds"] > 0
        assert all(_same_bits(Z[j], want[j]) for j in range(5))
        assert _same_bits(sh.score(cols[0])[0], want[0])
        xv, za, zb = sh.vecM(cols[1]), sh.vecN(), sh.vecN()
        sh.score_dev([xv, xv], [za, zb])                                # inputs may repeat
        assert _same_bits(za.download(), want[1]) and _same_bits(zb.download(), want[1])


# ---- 2. held to something outside the kernels ----------------------------------------------------------------------------------------
def test_first_and_last_column_are_held_to_the_integer_restatement():
    cs = _case("ragged")
    planes = bx.planes(cs["bed"], cs["N"], cs["M"], cs["present"])
    with _shard(cs) as sh:
        mave, msig = sh.marker_stats()
        cols = _columns(cs, sh, 17)
        got = _score(sh, cols)
        info = sh.score_info()
        assert info["path"] == "kernel" and info["passes"] == -(-17 // info["cols_per_pass"]) >= 2, info
        for j in (0, 16):
            S = bx.ax1_sums(planes, mave, msig, cols[j])
            assert bx.lo_exact(S["lo"])
            run = bx.find_K0(S, got[j], cs["N"], cs["present"])
            exact, bound = bx.exact_K0(mave, S["c"]), bx.k0_bound(mave, S["c"])
            near = run.nearest(exact)
            print("column %d: %d doubles reproduce every entry; nearest %+.2f ulp from the exact K0" %
                  (j, run.count, bx.ulps(near, exact) if near is not None else float("nan")))
            assert run.count > 0, "column %d: no single K0 reproduces every entry" % j
            assert abs(bx.Fraction(near) - exact) <= bound
        assert np.all(got[3] == 0.0) and np.all(got[15] == 0.0)        # the zero columns are exactly zero


# ---- 3. company and position do not matter -------------------------------------------------------------------------------------------
def test_position_and_neighbours_do_not_matter():
    cs = _case("even")
    with _shard(cs) as sh:
        cols = _columns(cs, sh, 17)
        want = _singles(sh, cols)
        probe = cols[1]
        rng = np.random.default_rng(5)
        for pos in (0, 7, 16):
            batch = [rng.standard_normal(cs["M"]) * 10.0 ** rng.integers(-6, 6) for _ in range(17)]
            batch[pos] = probe
            assert _same_bits(_score(sh, batch)[pos], want[1]), pos
        batch = list(cols[:6])
        batch[2] = cols[0].copy()
        batch[2][11] = np.nan
        batch[4] = cols[1].copy()
        batch[4][200] = np.inf
        got = _score(sh, batch)
        xv, zv = sh.vecM(batch[2]), sh.vecN()
        sh.ax_dev(xv, zv)
        alone = zv.download()
        pres = np.zeros(len(alone), dtype=bool)
        pres[:cs["N"]] = True if cs["present"] is None else cs["present"]
        for j in (2, 4):
            assert np.all(np.isnan(got[j][pres])) and np.all(got[j][~pres] == 0.0)
            assert np.array_equal(np.isnan(got[j]), np.isnan(alone))
        for j in (0, 1, 3, 5):
            assert _same_bits(got[j], want[j]), j


# ---- 4. fallback paths ------------------------------------------------------------------------------------------------------------------
def _full_mask(N):
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in range(N):
        m4[n >> 2] |= 1 << (n & 3)
    return m4


@pytest.mark.parametrize("what", ["two-stripe-sets", "mode2", "mode0", "forced-multi", "dosage8", "meth"])
def test_fallback_paths_report_themselves_and_keep_the_bits(what):
    cs = _case("ragged")
    if what in ("dosage8", "meth"):
        N, M = 515, 300
        sh = capi.Shard(N, M)
        if what == "meth":
            sh.synth_meth(3)
        else:
            sh.synth_dosage(3, 8)
        sh.set_mask(_full_mask(N), N)
        sh.compute_markers_statistics()
        rng = np.random.default_rng(9)
        cols = [rng.standard_normal(M) * 10.0 ** k for k in range(5)]
    else:
        sh = _shard(cs, layout={"two-stripe-sets": 1, "mode0": "raw"}.get(what, 2), mode={"mode2": 2, "mode0": 0}.get(what, 1))
        if what == "forced-multi":
            sh.force_multi(1)
        cols = _columns(cs, sh, 5)
    with sh:
        want = _singles(sh, cols)
        for C in (1, 2, 5):
            got = _score(sh, cols[:C])
            info = sh.score_info()
            assert info["path"] == "fallback" and info["columns"] == C and info["ksegs"] == 0, info
            assert all(_same_bits(got[j], want[j]) for j in range(C)), (what, C)
        assert any(np.any(w != 0) for w in want)


# ---- 5. the int32 bound ------------------------------------------------------------------------------------------------------------------
def test_no_segment_lets_an_int32_digit_sum_wrap():
    """N = 8 x M = 4 194 304 + 64: one marker more than a single K-segment may hold.  Column 1 is the adversarial vector of
    tests/test_gpu_segment_bound.py: marker 0 (monomorphic, a = 2) carries 2^53, every other marker is all-missing and carries
    -0x808080808080, so each adds -512 to digit column 0; the exact product is 0 unless a sum wraps."""
    N, M = 8, 4194304 + 64
    bed = np.full((M, 2), 0x55, dtype=np.uint8)
    bed[0, :] = 0x00
    adv = np.full(M, -141289400074368.0)
    adv[0] = 2.0 ** 53
    rng = np.random.default_rng(2)
    cols = [rng.standard_normal(M), adv, np.ones(M)]

    def make(env, upload):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            sh = capi.Shard(N, M)
            sh.set_layout(False, 2)
            if upload:
                sh.upload_bed(bed.reshape(-1))
            else:
                sh.synth_bed(7, 5000)                  # the refusal depends on the shape alone
            sh.compute_markers_statistics()
        return sh

    # (GV_AUTOTUNE=0: the one-vector products this is compared with run on the model's decomposition, without the seconds of its
    # on-device pick at this extreme shape; the bits do not depend on it)
    with make(dict(GV_SCORE_KERNEL="1", GV_AUTOTUNE="0"), True) as sh:
        mave, msig = sh.marker_stats()
        assert mave[0] == 2.0 and msig[0] == 1.0 and np.all(mave[1:] == 0.0) and np.all(msig[1:] == 1.0)
        want = _singles(sh, cols)
        got = _score(sh, cols)
        info = sh.score_info()
        assert info["path"] == "kernel" and info["ksegs"] >= 2, info
        assert all(_same_bits(got[j], want[j]) for j in range(3))
        assert np.all(got[1] == 0.0)
    with make(dict(GV_SCORE_KERNEL="1", GV_SCORE_KS="1"), False) as sh:
        xs, zs = [sh.vecM().fill(1.0) for _ in range(3)], [sh.vecN() for _ in range(3)]
        with pytest.raises(capi.GvError, match="GV_SCORE_KS=1.*int32"):
            sh.score_dev(xs, zs)


def test_gv_create_refuses_bad_overrides(monkeypatch):
    for k, v, msg in (("GV_SCORE_COLS", "5", "4, 8 or 16"), ("GV_SCORE_KS", "0", "positive integer"), ("GV_SCORE_KS", "65", "positive integer"),
                      ("GV_SCORE_KS", "x", "positive integer")):
        monkeypatch.setenv(k, v)
        with pytest.raises(capi.GvError, match=msg):
            capi.Shard(16, 64)
        monkeypatch.delenv(k)


# ---- 6. the context is left as it was ------------------------------------------------------------------------------------------------
def _free_device_memory():
    """hipMemGetInfo of the runtime the library has already loaded"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_the_context_is_left_as_it_was():
    cs = _case("even")
    with _shard(cs) as sh:
        cols = _columns(cs, sh, 16)
        xa, xb, za, zb, ov = sh.vecM(cols[0]), sh.vecM(cols[1]), sh.vecN(), sh.vecN(), sh.vecM()

        def probe():
            sh.ax_dev(xa, za)
            a1 = za.download()
            sh.ax2_dev(xa, xb, za, zb)
            a2 = (za.download(), zb.download())
            sh.lmmse_mult(xa, 1.3, 0.4, ov)
            return sh.decomp(), a1, a2[0], a2[1], ov.download()

        before = probe()
        xs, zs = [sh.vecM(x) for x in cols], [sh.vecN() for _ in cols]
        sh.score_dev(xs, zs)
        assert sh.score_info()["path"] == "kernel"
        first = zs[5].download()
        free1 = _free_device_memory()
        for _ in range(50):
            sh.score_dev(xs, zs)
        assert _same_bits(zs[5].download(), first)
        assert _free_device_memory() == free1
        after = probe()
        assert before[0] == after[0]
        assert all(_same_bits(b, a) for b, a in zip(before[1:], after[1:]))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message_and_the_context_stays_usable():
    cs = _case("ragged")
    with _shard(cs) as sh:
        cols = _columns(cs, sh, 3)
        want = _singles(sh, cols)
        xs, zs = [sh.vecM(x) for x in cols], [sh.vecN() for _ in cols]
        vp = capi.C.c_void_p
        sh.score_dev([], [])                                                       # C == 0 succeeds and does nothing
        with pytest.raises(capi.GvError, match="negative"):
            sh._ck(sh.L.gv_score_dev(sh.h, -1, (vp * 1)(), (vp * 1)()))
        with pytest.raises(capi.GvError, match="arrays of column handles are NULL"):
            sh._ck(sh.L.gv_score_dev(sh.h, 2, None, None))
        with pytest.raises(capi.GvError, match="handle of column 1 is NULL"):
            sh.score_dev([xs[0], None], zs[:2])
        with pytest.raises(capi.GvError, match="column 0: x must be M-space, out N-space"):
            sh.score_dev([zs[0]], [zs[1]])
        with pytest.raises(capi.GvError, match="column 1: x must be M-space, out N-space"):
            sh.score_dev(xs[:2], [zs[0], xs[2]])
        with pytest.raises(capi.GvError, match="column 2: two outputs are the same vector"):
            sh.score_dev(xs, [zs[0], zs[1], zs[0]])
        with pytest.raises(capi.GvError, match="negative"):
            sh._ck(sh.L.gv_score(sh.h, -2, None, None))
        with pytest.raises(capi.GvError, match="W or out is NULL"):
            sh._ck(sh.L.gv_score(sh.h, 2, None, None))
        got = _score(sh, cols)
        assert all(_same_bits(got[j], want[j]) for j in range(3))
    # marker statistics missing: refused as gv_ax_dev refuses it
    with capi.Shard(cs["N"], cs["M"]) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        xs, zs = [sh.vecM().fill(1.0) for _ in range(4)], [sh.vecN() for _ in range(4)]
        with pytest.raises(capi.GvError) as single:
            sh.ax_dev(xs[0], zs[0])
        with pytest.raises(capi.GvError) as batch:
            sh.score_dev(xs, zs)
        assert str(batch.value) == str(single.value) and "statistics" in str(batch.value)
