"""The fixed-point i8 MFMA route of 8-bit dosage codes (gv_set_dosage_route(ctx, 1): k_dm_max, k_dm_quant, k_dm_atx, k_dm_ax,
k_dm_fin_atx, k_dm_fin_ax of gv_dense_mfma.hip) held to the integer restatement of tests/dosage_fixed_restatement.py -- something
OUTSIDE the kernels, and exact -- BIT FOR BIT: tests/test_gpu_dosage_mfma.py compares the kernels with a long-double restatement at
1e-13 and with themselves, and a kernel that loses its lowest digit plane (3e-14) or truncates where it should round passes that.

Every output entry of gv_ax / gv_atx, of both slots of their two-vector forms and of gv_lmmse_mult equals the restatement, pad slots
are exact zeros; at every shape of dosage_fixed_cases.SHAPES (one per structural edge of the two streaming kernels), under the
library's own K-segments, one K-step per segment and a length between; for ordinary vectors, twelve decades of dynamic range and
digit-edge vectors on either side.  mu' is taken from the restatement (the device's is checked through mave, the only view of it),
msig from the device.  tests/test_dosage_fixed_cpu.py shows on these very inputs that each of six subtle mutants of the
restatement changes output bits at every shape from 63 x 63 on."""
import numpy as np
import pytest

import dosage_fixed_cases as dc
import dosage_fixed_restatement as fx
from gvamp_amd import capi
from test_gpu_dosage_mfma import shard

pytestmark = pytest.mark.gpu
SCALE = dc.SCALE
SETUPS = [(N, M, na, seg) for (N, M, na) in dc.SHAPES for seg in dc.SEGS]
_MEMO = {}


def _resident(cs, seg=None, transport=0):
    """route 1 in force on the codes of the case; msig from the device, mu' checked against the restatement's bit for bit"""
    sh = shard(cs["N"], cs["M"], seg)
    try:
        if transport:
            sh._ck(sh.L.gv_debug_force_multi(sh.h, transport, 0))
        sh.set_dosage_route(1)
        sh.upload_dosage(cs["B"], SCALE)
        if cs["with_na"]:
            sh.set_mask(cs["m4"], cs["nonas"])
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (1, 1)
        mave, msig = sh.marker_stats()
        assert np.array_equal(mave, SCALE * cs["mu"])          # k_dosage_stats: mave = scale mu', mu' = exact integer sum / nonas
    except BaseException:
        sh.close()
        raise
    return sh, msig


def _pad(sh, p):
    """an N-space vector as the C ABI takes it: 4 * gv_mbytes entries, zeros past N"""
    out = np.zeros(4 * sh.mbytes)
    out[:len(p)] = p
    return out


def _memo(cs, what, v, msig, fn):
    """a restated product is computed once per (case, vector, device statistics) and shared by the segment lengths and entry points"""
    key = (cs["N"], cs["M"], cs["with_na"], what, v.tobytes(), msig.tobytes())
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _ref_ax(cs, msig, x):
    return _memo(cs, "ax", x, msig, lambda: fx.ax(cs["B"], cs["mu"], msig, SCALE, x))


def _ref_atx(cs, msig, p):
    return _memo(cs, "atx", p, msig, lambda: fx.atx(cs["B"], cs["mu"], msig, SCALE, p))


def _same(what, got, ref):
    """bit for bit (NaN equals NaN: a slot with an entry that is not finite is NaN everywhere)"""
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0]
    print("%s: %d of %d entries differ" % (what, len(bad), len(ref)))
    assert np.array_equal(got, ref, equal_nan=True), (what, bad[:5], got[bad[:5]], ref[bad[:5]])


def _same_ax(what, z, ref, N):
    _same(what, z[:N], ref)
    assert len(z) >= N and not np.any(z[N:]), what          # exact zeros at the pad slots


def _check_edges(cs, msig, kind, x):
    """the weights as the DEVICE forms them (its msig) reach the digit edges too"""
    if kind.startswith("edge") and cs["M"] >= dc.SENSITIVE:
        dc.assert_edges(dc.edge_report(dc.weights(msig, x)), kind == "edge-top")


@pytest.mark.parametrize("N,M,with_na,seg", SETUPS)
def test_one_vector_products_equal_the_restatement(N, M, with_na, seg):
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs, seg)
    with sh:
        for kind in dc.KINDS:
            x, p = dc.x_vector(kind, cs, msig), dc.p_vector(kind, cs)
            _check_edges(cs, msig, kind, x)
            z, w = sh.Ax(x), sh.ATx(_pad(sh, p))
            _same_ax("Ax %s" % kind, z, _ref_ax(cs, msig, x), N)
            _same("ATx %s" % kind, w, _ref_atx(cs, msig, p))
            assert (np.any(z != 0) and np.any(w != 0)) or N == 1          # (the one row of 1 x 1 is constant: b - mu' == 0)


@pytest.mark.parametrize("N,M,with_na,seg", SETUPS)
def test_two_vector_products_each_slot_equals_the_restatement_of_its_own_vector(N, M, with_na, seg):
    """the exponents of the two slots are 20 apart and more (asserted): scal and the limb sums of a slot are its own"""
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs, seg)
    with sh:
        for ka, kb in (("normal", "edge-top"), ("edge-pow2", "decades")):
            xs, ps = [dc.x_vector(k, cs, msig) for k in (ka, kb)], [dc.p_vector(k, cs) for k in (ka, kb)]
            assert abs(fx.exponent(ps[0]) - fx.exponent(ps[1])) >= 20
            if M >= dc.SENSITIVE:
                assert abs(fx.exponent(dc.weights(msig, xs[0])) - fx.exponent(dc.weights(msig, xs[1]))) >= 20
            xa, xb, za, zb = sh.vecM(xs[0]), sh.vecM(xs[1]), sh.vecN(), sh.vecN()
            sh.ax2_dev(xa, xb, za, zb)
            pa, pb, wa, wb = sh.vecN(_pad(sh, ps[0])), sh.vecN(_pad(sh, ps[1])), sh.vecM(), sh.vecM()
            sh.atx2_dev(pa, pb, wa, wb)
            for slot, (k, z, w) in enumerate(((ka, za, wa), (kb, zb, wb))):
                _same_ax("ax2_dev slot %d %s" % (slot, k), z.download(), _ref_ax(cs, msig, xs[slot]), N)
                _same("atx2_dev slot %d %s" % (slot, k), w.download(), _ref_atx(cs, msig, ps[slot]))
            for v in (xa, xb, za, zb, pa, pb, wa, wb):
                v.free()


@pytest.mark.parametrize("N,M,with_na,seg", SETUPS)
def test_lmmse_mult_equals_the_restated_composition(N, M, with_na, seg):
    """lmmse_device: z = Ax(x) into an N-space work vector (zeros at the pad slots, which ATx does not read), then ATx(z) whose epilogue
    k_dm_fin_atx forms fma(tau, w, gam2 * x) -- fx.lmmse restates that"""
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs, seg)
    with sh:
        for kind in ("normal", "edge-top"):
            x = dc.x_vector(kind, cs, msig)
            xv, out = sh.vecM(x), sh.vecM()
            sh.lmmse_mult(xv, dc.TAU, dc.GAM2, out)
            ref = _memo(cs, "lmmse", x, msig, lambda: fx.lmmse(cs["B"], cs["mu"], msig, SCALE, x, dc.TAU, dc.GAM2))
            _same("lmmse_mult %s" % kind, out.download(), ref)
            assert np.any(ref != 0) or N == 1


@pytest.mark.parametrize("seg", dc.SEGS)
def test_under_the_multi_rank_transport_every_product_equals_the_restatement(seg):
    """gv_debug_force_multi(h, 1, 0): Ax applies 1.0 inside and 1 / sqrt(N) after the exchange -- the same bits"""
    N, M, with_na = 1003, 700, True
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs, seg, transport=1)
    with sh:
        for kind in dc.KINDS:
            x, p = dc.x_vector(kind, cs, msig), dc.p_vector(kind, cs)
            _same_ax("Ax %s" % kind, sh.Ax(x), _ref_ax(cs, msig, x), N)
            _same("ATx %s" % kind, sh.ATx(_pad(sh, p)), _ref_atx(cs, msig, p))
        xs, ps = [dc.x_vector(k, cs, msig) for k in ("edge-pow2", "normal")], [dc.p_vector(k, cs) for k in ("edge-pow2", "normal")]
        xa, xb, za, zb = sh.vecM(xs[0]), sh.vecM(xs[1]), sh.vecN(), sh.vecN()
        sh.ax2_dev(xa, xb, za, zb)
        pa, pb, wa, wb = sh.vecN(_pad(sh, ps[0])), sh.vecN(_pad(sh, ps[1])), sh.vecM(), sh.vecM()
        sh.atx2_dev(pa, pb, wa, wb)
        for slot, (z, w) in enumerate(((za, wa), (zb, wb))):
            _same_ax("ax2_dev slot %d" % slot, z.download(), _ref_ax(cs, msig, xs[slot]), N)
            _same("atx2_dev slot %d" % slot, w.download(), _ref_atx(cs, msig, ps[slot]))
        out = sh.vecM()
        sh.lmmse_mult(xb, dc.TAU, dc.GAM2, out)
        _same("lmmse_mult", out.download(), _memo(cs, "lmmse", xs[1], msig,
                                                  lambda: fx.lmmse(cs["B"], cs["mu"], msig, SCALE, xs[1], dc.TAU, dc.GAM2)))


@pytest.mark.parametrize("N,M,with_na", [(63, 17, False), (130, 70, True)])
def test_special_vectors(N, M, with_na):
    """a zero vector gives exact zeros; one NaN or one infinity gives NaN in every entry of that slot (pad slots of Ax stay zero) and
    leaves the other slot of a two-vector call untouched, bit for bit; max|v| < 2^-946 meets the cap of the multiplier (sh > 1000 in
    k_dm_quant), which fx.exponent restates; subnormal entries beside a normal maximum"""
    cs = dc.case(N, M, with_na)
    sh, msig = _resident(cs)
    with sh:
        for kind in dc.SPECIAL:
            x, p = dc.x_vector(kind, cs, msig), dc.p_vector(kind, cs)
            z, w = sh.Ax(x), sh.ATx(_pad(sh, p))
            rz, rw = _ref_ax(cs, msig, x), _ref_atx(cs, msig, p)
            _same_ax("Ax %s" % kind, z, rz, N)
            _same("ATx %s" % kind, w, rw)
            if kind == "zero":
                assert not np.any(z) and not np.any(w)
            elif kind in ("nan", "inf"):
                assert np.all(np.isnan(z[:N])) and np.all(np.isnan(w))
            else:
                assert np.any(z != 0) and np.any(w != 0) and np.all(np.isfinite(z)) and np.all(np.isfinite(w))
            if kind == "tiny":
                assert fx.exponent(p) == fx.E_MIN and fx.exponent(dc.weights(msig, x)) == fx.E_MIN
            # beside an ordinary vector in the other slot, either way round
            xo, po = dc.x_vector("normal", cs, msig), dc.p_vector("normal", cs)
            for first in (True, False):
                xs, ps = ((x, xo), (p, po)) if first else ((xo, x), (po, p))
                xa, xb, za, zb = sh.vecM(xs[0]), sh.vecM(xs[1]), sh.vecN(), sh.vecN()
                sh.ax2_dev(xa, xb, za, zb)
                pa, pb, wa, wb = sh.vecN(_pad(sh, ps[0])), sh.vecN(_pad(sh, ps[1])), sh.vecM(), sh.vecM()
                sh.atx2_dev(pa, pb, wa, wb)
                for slot, (zv, wv) in enumerate(((za, wa), (zb, wb))):
                    _same_ax("ax2_dev %s slot %d" % (kind, slot), zv.download(), _ref_ax(cs, msig, xs[slot]), N)
                    _same("atx2_dev %s slot %d" % (kind, slot), wv.download(), _ref_atx(cs, msig, ps[slot]))
                for v in (xa, xb, za, zb, pa, pb, wa, wb):
                    v.free()
