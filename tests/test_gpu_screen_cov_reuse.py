"""The cached covariate side of the adjusted screen (gv_screen_cov_set: the basis Q and the per-marker v, DESIGN.md sections 22 and 26)
on a context that is REUSED, in the manner of tests/test_gpu_context_reuse.py: every case

  1. runs gv_screen_cov_set and gv_screen_cov_dev on the context in the OLD state (the cache is warm),
  2. changes one input -- the mask, the standardisation, the data set, the dimensions --, makes the calls include/gvamp.h documents for
     it, and shows that gv_screen_cov_dev then REFUSES by naming gv_screen_cov_set: it never answers from the previous state,
  3. calls gv_screen_cov_set and compares all five outputs with those of a context created for the new state by np.array_equal on the
     bits -- no tolerance,
  4. and shows that the fresh OLD and fresh NEW answers differ, so that a stale answer could not pass (the standardisation case goes
     through alpha_scale = 0.5, which both calls refuse, and back: old and new agree there, and the leg is still compared).

Shapes: N = 1203 is ragged modulo 4, 16, 64 and 256; M = 650 spans eleven 64-marker row groups; the second set of dimensions is (515, 257)."""
import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
N0, M0, N1, M1 = 1203, 650, 515, 257
NAMES = ("r", "t", "p", "beta", "se")
_CACHE = {}


@pytest.fixture(autouse=True)
def _no_tune_cache(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


def _mask(N, with_na):
    na = np.ones(N, dtype=bool)
    if with_na:
        na[3::7] = False
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    idx = np.nonzero(na)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return m4, int(na.sum())


def _inputs(N):
    """(Y, Cov): 3 raw phenotype and 3 raw covariate columns for N individuals (values at NA individuals are ignored by the library)"""
    if ("in", N) not in _CACHE:
        rng = np.random.default_rng(N)
        Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N), (rng.random(N) < 0.4).astype(float)])
        _CACHE[("in", N)] = (rng.standard_normal((3, N)) + np.array([[0.5, 0.02, 0.0], [0.0, 0.1, 1.0], [1.0, 0.0, -1.0]]) @ Cov, Cov)
    return _CACHE[("in", N)]


def _enter(sh, st, upload=True):
    """the documented calls that bring a context of the right dimensions into state st = (seed, masked)"""
    seed, masked = st
    if upload:
        sh.upload_bed(synth.synth_bed(sh.N, sh.M, seed=seed, miss_ppm=10000))
    sh.set_mask(*_mask(sh.N, masked))
    sh.compute_markers_statistics()


def _fresh(dims, st):
    key = ("fresh", dims, st)
    if key not in _CACHE:
        with capi.Shard(*dims) as sh:
            sh.set_layout(False, 2)
            _enter(sh, st)
            _CACHE[key] = sh.screen_cov(*_inputs(dims[0]))
    return _CACHE[key]


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in NAMES)


def _refuses(sh):
    Y = _inputs(sh.N)[0]
    ys, rs = [sh.vecN(sh._padN(y)) for y in Y], [sh.vecM().fill(7.0) for _ in Y]
    with pytest.raises(capi.GvError, match="gv_screen_cov_set must be called first"):
        sh.screen_cov_dev(ys, rs)
    assert all(np.all(v.download() == 7.0) for v in rs) and sh.screen_cov_info()["K"] is None
    for v in ys + rs:
        v.free()


OLD = (1, False)


@pytest.mark.parametrize("change", ["mask", "standardisation", "data set", "dimensions"])
def test_a_changed_input_drops_the_cached_state_and_a_new_set_equals_a_fresh_context(change):
    dims_new = (N1, M1) if change == "dimensions" else (N0, M0)
    new = {"mask": (1, True), "standardisation": OLD, "data set": (2, False), "dimensions": (1, False)}[change]
    with capi.Shard(N0, M0) as sh:
        sh.set_layout(False, 2)
        _enter(sh, OLD)
        assert _same(sh.screen_cov(*_inputs(N0)), _fresh((N0, M0), OLD))
        if change == "mask":
            sh.set_mask(*_mask(N0, True))
            with pytest.raises(capi.GvError, match="marker statistics must be set first"):
                sh.screen_cov(_inputs(N0)[0], False)
            sh.compute_markers_statistics()
        elif change == "standardisation":
            sh.compute_markers_statistics(0.5)
            with pytest.raises(capi.GvError, match="alpha_scale = 1"):
                sh.screen_cov(_inputs(N0)[0], False)
            sh.compute_markers_statistics()
        elif change == "data set":
            _enter(sh, new)
        else:
            sh.set_dims(N1, M1)
            _enter(sh, new)
        _refuses(sh)
        Y, Cov = _inputs(dims_new[0])
        got = sh.screen_cov(Y, Cov)
        assert sh.screen_cov_info()["K"] == 3
        assert _same(got, sh.screen_cov(Y, False))
    fresh_new = _fresh(dims_new, new)
    assert _same(got, fresh_new)
    if change in ("mask", "data set"):
        old = _fresh((N0, M0), OLD)
        assert not any(np.array_equal(old[k], fresh_new[k], equal_nan=True) for k in NAMES)
