"""The z-side kernels of --model robust (vamp_Huber.cpp): gv_huber_denoise (g1_Huber and its derivative) and gv_huber_delta (the
closed-form delta_H objective) against the numpy restatement in tests/robust_restatement.py."""
import numpy as np
import pytest

from gvamp_amd import capi

import robust_restatement as rr

pytestmark = pytest.mark.gpu


def _case(N, seed, tau1, d):
    """p1, y over the padded N-space; individuals 0..5 sit on the three branches with |w| == thr exactly, every 11th has y = 0
    (an NA phenotype after filter_pheno), the rest spread over the tails"""
    rng = np.random.default_rng(seed)
    npad = 4 * ((N + 3) // 4)
    p1, y = np.zeros(npad), np.zeros(npad)
    p1[:N] = rng.standard_normal(N) * np.where(rng.random(N) < 0.05, 20.0, 1.0)
    y[:N] = rng.standard_normal(N) * 1.5
    y[:N][::11] = 0.0
    thr = (1 + 1.0 / tau1) * d
    fixed = [(0.0, thr), (0.0, -thr), (0.0, 0.5 * thr), (0.0, 3 * thr), (0.0, -3 * thr), (1.0, 1.0)]
    for i, (p, yy) in enumerate(fixed[:N]):
        p1[i], y[i] = p, yy
    return p1, y


@pytest.mark.parametrize("N", [1, 255, 257, 100003])
def test_huber_denoiser_vs_numpy(N):
    for tau1, d in ((1e-8, 1e-3), (0.8, 0.5), (2.5, 1e-4), (40.0, 3.0)):
        p1, y = _case(N, N + 1, tau1, d)
        want, der = rr.g1_huber(p1[:N], tau1, d, y[:N])
        with capi.Shard(N, 8) as sh:
            dp, dy, dz = sh.vecN(p1), sh.vecN(y), sh.vecN(np.full(p1.size, 7.0))
            sums = sh.huber_denoise(dp, dy, tau1, d, dz)
            z = dz.download()
            assert np.allclose(z[:N], want, rtol=1e-15, atol=0), (tau1, d)
            assert np.all(z[N:] == 0.0)                                      # pad slots: exact zeros
            assert np.isclose(sums[0], der.sum(), rtol=1e-13, atol=0), (tau1, d)
            assert np.isclose(sums[1], ((want - p1[:N]) ** 2).sum(), rtol=1e-13, atol=0), (tau1, d)
            if N >= 6:                                                       # |w| == thr is on the inside branch
                assert z[0] == y[0] - y[0] / (1 + 1.0 / tau1) and z[1] == y[1] - y[1] / (1 + 1.0 / tau1)
            assert np.array_equal(dp.download(), p1) and np.array_equal(dy.download(), y)   # operands untouched


@pytest.mark.parametrize("N", [1, 257, 100003])
def test_huber_delta_objective_vs_numpy_and_reproducible(N):
    for tau1 in (1e-8, 0.3, 2.5, 1e4):
        p1, y = _case(N, 3 * N, tau1, 0.1)
        want = rr.delta_objective(p1[:N], y[:N], tau1)
        with capi.Shard(N, 8) as sh:
            dp, dy = sh.vecN(p1), sh.vecN(y)
            got = sh.huber_delta(dp, dy, tau1, rr.GRID)
            again = sh.huber_delta(dp, dy, tau1, rr.GRID)
        assert np.allclose(got, want, rtol=1e-12, atol=0), (tau1, np.max(np.abs(got - want) / np.abs(want)))
        assert rr.first_min(got) == rr.first_min(want), tau1
        assert np.array_equal(got, again)                                    # fixed-order reduction: same bits


def test_huber_delta_picks_larger_delta_for_gaussian_than_contaminated_noise():
    N = 20000
    rng = np.random.default_rng(5)
    noise = {"gaussian": rng.standard_normal(N),
             "contaminated": np.where(rng.random(N) < 0.1, 10.0, 1.0) * rng.standard_normal(N)}
    pick = {}
    with capi.Shard(N, 8) as sh:
        dp = sh.vecN(np.zeros(4 * sh.mbytes))
        for k, e in noise.items():
            y = np.zeros(4 * sh.mbytes)
            y[:N] = e
            pick[k] = rr.first_min(sh.huber_delta(dp, sh.vecN(y), 100.0, rr.GRID))
    assert pick["gaussian"] > pick["contaminated"] > rr.GRID[0], pick


def test_huber_entry_points_refuse_bad_arguments():
    N, M = 100, 8
    with capi.Shard(N, M) as sh:
        pn, yn, zn, xm = sh.vecN(), sh.vecN(), sh.vecN(), sh.vecM()
        with pytest.raises(capi.GvError, match="N-space"):
            sh.huber_denoise(xm, yn, 1.0, 0.1, zn)
        with pytest.raises(capi.GvError, match="N-space"):
            sh.huber_delta(pn, xm, 1.0, rr.GRID)
        with pytest.raises(capi.GvError, match="16"):
            sh.huber_delta(pn, yn, 1.0, np.linspace(0.1, 2, 17))
        with pytest.raises(capi.GvError, match="positive"):
            sh.huber_delta(pn, yn, 1.0, [0.1, 0.0])
