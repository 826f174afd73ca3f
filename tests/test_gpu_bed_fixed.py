"""The bed fixed-point products of kernel modes 1 and 2 (k_quant, k_mfma_matvec / k_mfma_tile, k_fin_ax / k_fin_atx and their _wide
twins) held to the integer restatement of tests/bed_fixed_restatement.py -- something OUTSIDE the kernels, and exact: every other
bit-identity test compares the kernels with each other, and the fp64 oracle at 1e-12 cannot see a wrong lowest digit (1e-13).

* mode 2, Ax and ATx: every output entry equals the restatement bit for bit (pads and NA rows included);
* mode 1: the ordered fp64 reductions K0 = sum mave c (Ax) and P = sum p (ATx) are the only freedom -- there must be ONE double that
  reproduces every entry, within the summation bound of the exact sum (how many do, and their distance in ulps, is printed);
* lmmse_mult and the two-vector entry points likewise;
* both resident layouts, the library's pick and a pinned three-segment decomposition on all four classes (gather_pieces adds pieces).

tests/test_bed_fixed_cpu.py shows on these very inputs that a dropped lowest digit or a truncating quantiser changes at least half
of the entries of every product compared here."""
import math

import numpy as np
import pytest

import bed_fixed_restatement as bx
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
TAU, GAM2 = 1.3, 0.4
SETUPS = [(layout, decomp) for layout in (1, 2) for decomp in ("pick", "ks3")]
_CACHE = {}


@pytest.fixture(autouse=True)
def _no_tune_cache(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


def _case(name):
    if name not in _CACHE:
        cs = bx.case(name)
        cs["planes"] = bx.planes(cs["bed"], cs["N"], cs["M"], cs["present"])
        _CACHE[name] = cs
    return _CACHE[name]


def _memo(key, mave, msig, fn):
    """restated quantities are computed once per (input, device statistics) and shared by the layouts and decompositions"""
    key = key + (mave.tobytes(), msig.tobytes())
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _shard(cs, layout, decomp, mode):
    """decomp "ks3": three K-segments on all four classes (gv_set_decomp).  The partial-sum buffer of a shard this small has room for
    the tuner's own candidates only (two pieces), so the context is planned under GV_KS_M = GV_KS_N = 3 -- read at gv_set_dims and at
    ingest -- which sizes the buffer for three"""
    with pytest.MonkeyPatch.context() as mp:
        if decomp == "ks3":
            mp.setenv("GV_KS_M", "3")
            mp.setenv("GV_KS_N", "3")
        sh = capi.Shard(cs["N"], cs["M"])
        sh.set_layout(False, layout)                     # 1: two stripe sets, 2: one tile layout
        sh.set_kernel_mode(mode)
        sh.upload_bed(cs["bed"])
    if cs["m4"] is not None:
        sh.set_mask(cs["m4"], cs["nonas"])
    sh.compute_markers_statistics()
    if decomp == "ks3":
        for cls in ("atx", "atx2", "ax", "ax2"):
            sh.set_decomp(cls, ks=3)
        assert all(v.get("ks") == 3 for v in sh.decomp().values()), sh.decomp()
    mave, msig = sh.marker_stats()
    assert mave[bx.MONO] == 2.0 and msig[bx.MONO] == 1.0 and mave[bx.ALLMISS] == 0.0 and msig[bx.ALLMISS] == 1.0
    return sh, mave, msig


def _report(what, run, exact, bound):
    """run: every double that reproduces all output entries (bx.find_scalar).  It must not be empty, and must hold a double within the
    summation bound of the exact sum (the device's own scalar is in the run and has to be)"""
    near = run.nearest(exact)
    print("%s: %d doubles reproduce the pinning entry, %d reproduce every entry; the nearest is %+.2f ulp (%.3g) from the exact sum, bound "
          "%.3g ulp (%.3g)" % (what, run.pinned, run.count, bx.ulps(near, exact) if near is not None else math.nan,
                               abs(float(bx.Fraction(near) - exact)) if near is not None else math.nan,
                               float(bound / bx.Fraction(math.ulp(near))) if near else math.nan, float(bound)))
    assert run.count > 0, what + ": no single double reproduces every output entry"
    assert abs(bx.Fraction(near) - exact) <= bound, what + ": the scalar is outside its summation bound"


def _check_ax1(cs, what, x, z, mave, msig, key):
    S = _memo(key, mave, msig, lambda: bx.ax1_sums(cs["planes"], mave, msig, x))
    assert bx.lo_exact(S["lo"])
    if not np.any(x):
        assert np.all(z == 0), what
        assert np.array_equal(bx.ax1_epilogue(S, 0.0, cs["N"], cs["present"]), z)
        return
    _report(what, bx.find_K0(S, z, cs["N"], cs["present"]), bx.exact_K0(mave, S["c"]), bx.k0_bound(mave, S["c"]))


def _check_atx1(cs, what, p, w, mave, msig, key, lm=None):
    S = _memo(key, mave, msig, lambda: bx.atx1_sums(cs["planes"], p, cs["N"], cs["present"]))
    assert bx.lo_exact(S["lo"]) and S["sm"][bx.MONO] == 0.0
    if not np.any(p):
        assert np.all(w == 0), what
        assert np.array_equal(bx.atx1_epilogue(S, 0.0, mave, msig, cs["N"]), w)
        return
    _report(what, bx.find_P(S, w, mave, msig, cs["N"], bx.MONO, lm), bx.exact_P(p), bx.p_bound(p, cs["N"]))


@pytest.mark.parametrize("layout,decomp", SETUPS)
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_mode2_every_entry_equals_the_restatement(name, layout, decomp):
    cs = _case(name)
    sh, mave, msig = _shard(cs, layout, decomp, 2)
    with sh:
        for kind in (1, 2, 3, 4):
            x, p = bx.vector_x(cs, kind, 2, mave, msig), bx.vector_p(cs, kind)
            z, w = sh.Ax(x), sh.ATx(p)
            rz = _memo((name, "ax2", kind), mave, msig, lambda: bx.ax2(cs["planes"], mave, msig, x, cs["N"], cs["present"]))
            rw = _memo((name, "atx2", kind), mave, msig, lambda: bx.atx2(cs["planes"], mave, msig, p, cs["N"], cs["present"]))
            bad_z, bad_w = np.nonzero(z != rz)[0], np.nonzero(w != rw)[0]
            print("mode 2 %s vector %d: Ax %d of %d entries differ, ATx %d of %d" % (name, kind, len(bad_z), len(z), len(bad_w), len(w)))
            assert np.array_equal(z, rz), (kind, bad_z[:5], z[bad_z[:5]], rz[bad_z[:5]])
            assert np.array_equal(w, rw), (kind, bad_w[:5], w[bad_w[:5]], rw[bad_w[:5]])
            if kind == 4:
                assert np.all(z == 0) and np.all(w == 0)
            else:
                assert np.any(z != 0) and np.any(w != 0)


@pytest.mark.parametrize("layout,decomp", SETUPS)
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_mode1_ax_one_K0_reproduces_every_entry(name, layout, decomp):
    cs = _case(name)
    sh, mave, msig = _shard(cs, layout, decomp, 1)
    with sh:
        for kind in (1, 2, 3, 4):
            x = bx.vector_x(cs, kind, 1, mave, msig)
            _check_ax1(cs, "mode 1 Ax %s vector %d" % (name, kind), x, sh.Ax(x), mave, msig, (name, "ax1", kind))


@pytest.mark.parametrize("layout,decomp", SETUPS)
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_mode1_atx_one_P_reproduces_every_marker(name, layout, decomp):
    cs = _case(name)
    sh, mave, msig = _shard(cs, layout, decomp, 1)
    with sh:
        for kind in (1, 2, 3, 4):
            p = bx.vector_p(cs, kind)
            _check_atx1(cs, "mode 1 ATx %s vector %d" % (name, kind), p, sh.ATx(p), mave, msig, (name, "atx1", kind))


@pytest.mark.parametrize("layout,decomp", SETUPS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_lmmse_mult_is_the_restated_atx_of_the_device_ax(name, mode, layout, decomp):
    """out = fma(tau, ATx(z), gam2 x) with z = Ax(x) taken from the device (that Ax inside lmmse_mult is the plain Ax is shown by the
    existing tests)"""
    cs = _case(name)
    sh, mave, msig = _shard(cs, layout, decomp, mode)
    with sh:
        x = bx.vector_x(cs, 1, mode, mave, msig)
        xv, zv, ov = sh.vecM(x), sh.vecN(), sh.vecM()
        sh.ax_dev(xv, zv)
        sh.lmmse_mult(xv, TAU, GAM2, ov)
        z, out = zv.download(), ov.download()
        assert np.any(z != 0)
        if mode == 2:
            r = bx.atx2(cs["planes"], mave, msig, z, cs["N"], cs["present"])
            assert np.array_equal(out, bx.lmmse(TAU, r, GAM2, x))
        else:
            _check_atx1(cs, "mode 1 lmmse_mult %s" % name, z, out, mave, msig, (name, "lmmse", z.tobytes()), lm=(TAU, GAM2, x))


@pytest.mark.parametrize("layout,decomp", SETUPS)
@pytest.mark.parametrize("mode", [1, 2])
def test_two_vector_entry_points_each_slot_has_its_own_exponent_and_scalar(mode, layout, decomp):
    cs = _case("ragged")
    sh, mave, msig = _shard(cs, layout, decomp, mode)
    with sh:
        xs = [bx.vector_x(cs, kind, mode, mave, msig) for kind in (1, 2)]
        ps = [bx.vector_p(cs, kind) for kind in (1, 2)]
        assert bx.exponent(ps[0]) != bx.exponent(ps[1])
        xa, xb, za, zb = sh.vecM(xs[0]), sh.vecM(xs[1]), sh.vecN(), sh.vecN()
        sh.ax2_dev(xa, xb, za, zb)
        pa, pb, wa, wb = sh.vecN(ps[0]), sh.vecN(ps[1]), sh.vecM(), sh.vecM()
        sh.atx2_dev(pa, pb, wa, wb)
        for slot, (kind, z, w) in enumerate(((1, za.download(), wa.download()), (2, zb.download(), wb.download()))):
            x, p = xs[slot], ps[slot]
            if mode == 2:
                rz = _memo(("ragged", "ax2", kind), mave, msig, lambda: bx.ax2(cs["planes"], mave, msig, x, cs["N"], cs["present"]))
                rw = _memo(("ragged", "atx2", kind), mave, msig, lambda: bx.atx2(cs["planes"], mave, msig, p, cs["N"], cs["present"]))
                assert np.array_equal(z, rz) and np.array_equal(w, rw), slot
            else:
                _check_ax1(cs, "mode 1 ax2_dev slot %d" % slot, x, z, mave, msig, ("ragged", "ax1", kind))
                _check_atx1(cs, "mode 1 atx2_dev slot %d" % slot, p, w, mave, msig, ("ragged", "atx1", kind))
