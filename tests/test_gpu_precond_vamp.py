"""VAMP with the LD-block preconditioner (--cg-precond ld): the linear loop on LD genotypes at fuse levels
0, 1 and 4 against the oracle's scalar run, bin_class and robust against their scalar runs, independent genotypes, forced-multi
bit-identity, and the drivers' refusals."""
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, hostapi, synth
from test_gpu_forced_multi import _check_all, _trace

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]
KW = dict(iterations=6, CG_max_iter=400, rho=0.5, seed=9, gam1=1e-8, gamw=2.0, stop_criteria_thr=1e-12)


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _passes(r, first=1):
    return sum(t["n_ax_pass"] + t["n_atx_pass"] for t in r.trace[first:])


def _close(r, ref, what, tol=1e-4):
    assert r.niter == ref.niter, what
    for it in range(r.niter):
        t, o = r.trace[it], ref.trace[it]
        assert rel(r.x1[it], ref.x1[it]) < tol and rel(r.x2[it], ref.x2[it]) < tol, (what, it, rel(r.x1[it], ref.x1[it]),
                                                                                      rel(r.x2[it], ref.x2[it]))
        assert np.isclose(t["gamw"], o["gamw"], rtol=tol) and np.isclose(t["alpha2"], o["alpha2"], rtol=tol), (what, it)


@pytest.mark.parametrize("ld_block", [64, 48])
def test_linear_vamp_on_ld_data_against_the_oracle(oracle, ld_block):
    N, M = 2000, 5000
    bed = synth.synth_bed(N, M, seed=77, miss_ppm=5000, ld_block=ld_block, ld_ppm=900000)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        beta, y = hostapi.sim_phen(sh, 0.5, max(1, M // 50), 9)
        scalar4 = hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, fuse_solves=4, **KW)
        runs = {f: hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, fuse_solves=f, cg_precond="ld", **KW)
                for f in (0, 1, 4)}
    ref = oracle.infere(bed, N, M, y, PROBS, VARS, true_signal=beta, **KW)
    # every scalar solve converged below the cap, or the comparison means nothing
    assert all(t["cg_iters"] < KW["CG_max_iter"] and t["onsager_iters"] < KW["CG_max_iter"] for t in ref.trace + scalar4.trace)
    assert max(t["cg_iters"] for t in ref.trace) >= 12
    c_ref = np.corrcoef(ref.x_est, beta)[0, 1]
    for f, r in runs.items():
        _close(r, ref, "ld fuse %d" % f)
        assert abs(np.corrcoef(r.x_est, beta)[0, 1] - c_ref) < 1e-3
        assert all(t["probe_product"] == 0 for t in r.trace), f
    assert all(np.array_equal(runs[1].x1[it], runs[0].x1[it]) for it in range(KW["iterations"]))
    assert _passes(runs[4]) <= 0.6 * _passes(scalar4), (_passes(runs[4]), _passes(scalar4))


@pytest.mark.parametrize("model", ["bin_class", "robust"])
def test_other_models_on_ld_data(model):
    N, M = 2000, 5000
    bed = synth.synth_bed(N, M, seed=78, miss_ppm=5000, ld_block=64, ld_ppm=900000)
    kw = dict(KW, fuse_solves=4, model=model)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        beta, y = hostapi.sim_phen(sh, 0.5, max(1, M // 50), 9)
        if model == "bin_class":
            y = (y > np.median(y)).astype(np.float64)
            kw["gamw"] = 1.0
        s = hostapi.infere_linear(sh, y, PROBS, VARS, **kw)
        l = hostapi.infere_linear(sh, y, PROBS, VARS, cg_precond="ld", **kw)
    assert all(t["cg_iters"] < KW["CG_max_iter"] for t in s.trace)
    _close(l, s, model)
    assert abs(np.corrcoef(l.x_est, beta)[0, 1] - np.corrcoef(s.x_est, beta)[0, 1]) < 1e-3
    assert _passes(l) < _passes(s), (_passes(l), _passes(s))


def test_independent_genotypes_cost_at_most_two_passes_more():
    N, M = 2000, 5000
    bed = synth.synth_bed(N, M, seed=79, miss_ppm=5000)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        beta, y = hostapi.sim_phen(sh, 0.5, max(1, M // 50), 9)
        s = hostapi.infere_linear(sh, y, PROBS, VARS, fuse_solves=4, **KW)
        l = hostapi.infere_linear(sh, y, PROBS, VARS, fuse_solves=4, cg_precond="ld", **KW)
    _close(l, s, "independent")
    assert _passes(l, 0) <= _passes(s, 0) + 2 * KW["iterations"], (_passes(l, 0), _passes(s, 0))


def test_forced_multi_and_host_driven_loop_are_bit_identical():
    N, M = 1501, 2000
    bed = synth.synth_bed(N, M, seed=80, miss_ppm=5000, ld_block=64, ld_ppm=900000)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        beta, y = hostapi.sim_phen(sh, 0.5, max(1, M // 50), 9)
        kw = dict(KW, iterations=4, fuse_solves=4, cg_precond="ld", cg_precond_window=64)

        def run():
            return _trace(hostapi.infere_linear(sh, y, PROBS, VARS, **kw))

        _check_all(sh, run)


def test_hostapi_and_drivers_refuse(tmp_path):
    N, M = 600, 512
    with capi.Shard(N, M) as sh:
        sh.upload_bed(synth.synth_bed(N, M, seed=1, miss_ppm=5000))
        y = np.random.default_rng(0).standard_normal(N)
        with pytest.raises(capi.GvError, match="cg_precond"):
            hostapi.infere_linear(sh, y, PROBS, VARS, cg_precond="block")
        with pytest.raises(capi.GvError, match="cg_precond_window"):
            hostapi.infere_linear(sh, y, PROBS, VARS, cg_precond="ld", cg_precond_window=96)
        with pytest.raises(capi.GvError, match="use-XXT-denoiser"):
            hostapi.infere_linear(sh, y, PROBS, VARS, cg_precond="ld", use_XXT_denoiser=1)
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_sim_meth")
    res = subprocess.run([exe, "--bed-file", str(tmp_path / "m.bin"), "--N", "300", "--Mt", "400", "--out-dir", str(tmp_path) + "/",
                          "--out-name", "m", "--iterations", "1", "--num-mix-comp", "2", "--probs", "0.9,0.1", "--vars", "0,0.01",
                          "--CG-max-iter", "10", "--cg-precond", "ld"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 1 and "FATAL" in res.stdout and "methylation" in res.stdout, res.stdout[-2000:]
