"""The screens on dosage data on a context that is REUSED (include/gvamp.h, the table of derived state; DESIGN.md sections 22 and 29), in
the manner of tests/test_gpu_screen_cov_reuse.py.  Two rows of that table are held here:

  gv_set_screen_dosage   nothing goes stale: the option is read by every screen call, switching it changes no bit of any product or
                         statistic, and it outlives the data set and gv_set_dims.
  the per-marker q       (the variance input of the dosage screens, kept beside the mean codes) goes stale and is restored with the
                         marker statistics: after gv_set_mask, a new upload or gv_set_dims both screens REFUSE until gv_marker_stats
                         (and gv_screen_cov_set) has run again -- they never answer from the previous state -- and then answer bit for
                         bit as a context created for the new state; the fresh old and new answers differ, so a stale q could not pass.

A marker that is constant under one mask and varies under the other makes the NaN set itself depend on q being recomputed."""
import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
N0, M0, N1, M1 = 515, 300, 257, 130
NAMES = ("r", "t", "p", "beta", "se")
FLIP = 9            # constant among the individuals the mask keeps, varying among all
_CACHE = {}


def _mask(N, with_na):
    na = np.ones(N, dtype=bool)
    if with_na:
        na[3::7] = False
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    idx = np.nonzero(na)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return m4, int(na.sum())


def _codes(N, M, seed, bits):
    B = synth.synth_dosage_na(N, M, seed, bits, 30000).copy()
    B[FLIP] = 40
    B[FLIP, 3::7] = 90          # varies only at the individuals the mask leaves out
    return B


def _inputs(N):
    if N not in _CACHE:
        rng = np.random.default_rng(N)
        Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N), (rng.random(N) < 0.4).astype(float)])
        _CACHE[N] = (rng.standard_normal((3, N)) + np.array([[0.5, 0.02, 0.0], [0.0, 0.1, 1.0], [1.0, 0.0, -1.0]]) @ Cov, Cov)
    return _CACHE[N]


def _enter(sh, st, bits, upload=True):
    seed, masked = st
    if upload:
        sh.upload_dosage(_codes(sh.N, sh.M, seed, bits), 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0, missing=True)
    sh.set_mask(*_mask(sh.N, masked))
    sh.compute_markers_statistics()


def _both(sh):
    Y, Cov = _inputs(sh.N)
    out = sh.screen_cov(Y, Cov)
    out["marginal"] = np.stack(sh.screen(Y))
    return out


def _fresh(dims, st, bits):
    key = ("fresh", dims, st, bits)
    if key not in _CACHE:
        with capi.Shard(*dims) as sh:
            sh.set_screen_dosage(1)
            _enter(sh, st, bits)
            _CACHE[key] = _both(sh)
    return _CACHE[key]


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in NAMES + ("marginal",))


def _refuse_until_stats(sh):
    """marker statistics are gone: both screens refuse and write nothing"""
    Y = _inputs(sh.N)[0]
    ys, rs = [sh.vecN(sh._padN(y)) for y in Y], [sh.vecM().fill(7.0) for _ in Y]
    with pytest.raises(capi.GvError, match="marker statistics must be set first"):
        sh.screen_dev(ys, rs)
    with pytest.raises(capi.GvError, match="marker statistics must be set first"):
        sh.screen_cov_set(None)
    with pytest.raises(capi.GvError, match="marker statistics must be set first"):
        sh.screen_cov_dev(ys, rs)
    assert all(np.all(v.download() == 7.0) for v in rs)
    for v in ys + rs:
        v.free()


def _refuse_until_set(sh):
    Y = _inputs(sh.N)[0]
    ys, rs = [sh.vecN(sh._padN(y)) for y in Y], [sh.vecM().fill(7.0) for _ in Y]
    with pytest.raises(capi.GvError, match="gv_screen_cov_set must be called first"):
        sh.screen_cov_dev(ys, rs)
    assert all(np.all(v.download() == 7.0) for v in rs)
    for v in ys + rs:
        v.free()


OLD = (1, False)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("change", ["mask", "data set", "dimensions"])
def test_a_changed_input_makes_both_screens_refuse_and_the_new_answer_equals_a_fresh_context(change, bits):
    dims_new = (N1, M1) if change == "dimensions" else (N0, M0)
    new = {"mask": (1, True), "data set": (2, False), "dimensions": (1, False)}[change]
    with capi.Shard(N0, M0) as sh:
        sh.set_screen_dosage(1)
        _enter(sh, OLD, bits)
        assert _same(_both(sh), _fresh((N0, M0), OLD, bits))
        if change == "mask":
            sh.set_mask(*_mask(N0, True))
        elif change == "data set":
            sh.upload_dosage(_codes(N0, M0, new[0], bits), 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0, missing=True)
        else:
            sh.set_dims(N1, M1)
            assert sh.get_screen_dosage() == 1          # the option outlives the data set and the dimensions
            sh.upload_dosage(_codes(N1, M1, new[0], bits), 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0, missing=True)
        _refuse_until_stats(sh)
        _enter(sh, new, bits, upload=False)
        _refuse_until_set(sh)
        got = _both(sh)
    fresh_new = _fresh(dims_new, new, bits)
    assert _same(got, fresh_new)
    old = _fresh((N0, M0), OLD, bits)
    if change == "mask":
        # q of marker FLIP: positive among all individuals, exactly zero among the phenotyped -- decided from the new statistics
        assert np.all(np.isfinite(old["marginal"][0][:, FLIP])) and np.all(np.isnan(fresh_new["marginal"][:, :, FLIP]))
        assert all(np.all(np.isnan(fresh_new[k][:, FLIP])) for k in NAMES)
    if change in ("mask", "data set"):
        assert not any(np.array_equal(old[k], fresh_new[k], equal_nan=True) for k in NAMES + ("marginal",))


@pytest.mark.parametrize("route", [0, 1])
def test_switching_the_option_changes_no_bit_of_any_product(route):
    N, M = N0, M0
    rng = np.random.default_rng(4)
    x = rng.standard_normal(M)
    with capi.Shard(N, M) as sh:
        sh.set_dosage_route(route)
        sh.upload_dosage(synth.synth_dosage(N, M, 5, 8), 1.0 / 127.0)
        sh.set_mask(*_mask(N, True))
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (route, route)
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N) * sh._present

        def products():
            xv, zv, pv, wv, lm = sh.vecM(x), sh.vecN(), sh.vecN(p), sh.vecM(), sh.vecM()
            sh.ax_dev(xv, zv)
            sh.atx_dev(pv, wv)
            sh.lmmse_mult(xv, 1.7, 0.35, lm)
            outs = [sh.vecM() for _ in range(5)]
            sh.atxm_dev([pv] * 5, outs)
            res = [zv.download(), wv.download(), lm.download()] + [o.download() for o in outs] + list(sh.marker_stats())
            for v in [xv, zv, pv, wv, lm] + outs:
                v.free()
            return res

        off = products()
        sh.set_screen_dosage(1)
        on = products()
        sh.screen(rng.standard_normal((4, N)))
        sh.screen_cov(rng.standard_normal((4, N)), rng.standard_normal((2, N)))
        after = products()
        sh.set_screen_dosage(0)
        back = products()
    for other in (on, after, back):
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(off, other))
    assert all(np.any(a != 0) for a in off)
