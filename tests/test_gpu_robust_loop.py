"""--model robust end to end (vamp::infere_robust): the product's loop against the dense restatements of the
deferred schedule (robust_schedule_restatement.py) and of the reference's order (robust_restatement.py), the guard, the go/no-go
comparison with the linear model, forced-multi, host-transport shards, methylation data and the driver."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from gvamp_amd import capi, hostapi, synth

import robust_restatement as rr
import robust_schedule_restatement as rs
from test_gpu_forced_multi import _check_all, _shard, _trace
from test_gpu_meth import _bed_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
SPARSE = dict(frac=0.05, sd=0.2)
PROBS, VARS = [0.95, 0.05], [0.0, 0.04]
SCALARS = ("alpha1", "gam2", "alpha2", "beta1", "tau2", "tau1_next")


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _run(bed, N, M, y, probs, vars_, mode=1, **kw):
    with capi.Shard(N, M, anchor=(mode == 0)) as sh:
        sh.upload_bed(bed)
        sh.set_kernel_mode(mode)
        return hostapi.infere_linear(sh, y, probs, vars_, model="robust", **kw)


def _same_run(r, ref, deltas, N):
    assert r.niter == len(ref)
    assert [t["deltaH"] for t in r.trace] == deltas
    for it, (t, o) in enumerate(zip(r.trace, ref)):
        assert (t["cg_iters"], t["onsager_iters"]) == (o["cg"], o["ons"]), it
        for f in SCALARS:
            assert np.isclose(t[f], o[f], rtol=1e-6, atol=0), (it, f, t[f], o[f])
        assert rel(r.x2[it], o["x2"] / np.sqrt(N)) < 1e-7, it
    assert rel(r.x_est, ref[-1]["x1"]) < 1e-7                     # unscaled x1_hat (vamp_Huber.cpp:439)


@pytest.mark.parametrize("mode,fuse", [(0, 0), (0, 4), (1, 0), (1, 4)])
def test_deferred_schedule_vs_restatement(mode, fuse):
    N, M = 1001, 1500                                             # odd N: pad slots in every N-space vector
    bed, D, beta, y = rs.case(N, M, 11, 12, **SPARSE)
    kw = dict(iterations=6, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, stop_criteria_thr=1e-12)
    ref = rs.robust_run(D, y, PROBS, VARS, **kw)
    assert len(ref) == 6 and ref.stopped is None
    r = _run(bed, N, M, y, PROBS, VARS, mode, fuse_solves=fuse, **kw)
    _same_run(r, ref, [o["deltaH_applied"] for o in ref], N)
    assert np.corrcoef(r.x_est, beta)[0, 1] > 0.9


def test_reference_schedule_vs_robust_run():
    """the case of test_robust_cpu.py::test_restatement_converges_once_n_is_large, in the reference's order"""
    N, M = 20000, 500
    bed, D, beta, y = rs.case(N, M, 8, 9)
    kw = dict(iterations=6, CG_max_iter=30, rho=0.5, seed=4, gam1=1e-8, stop_criteria_thr=1e-12)
    ref = rr.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], **kw)
    r = _run(bed, N, M, y, [0.7, 0.3], [0.0, 0.09], huber_delta_schedule="reference", **kw)
    # robust_run records the delta_H its step at :259 left; the trace the one each iteration's g1_Huber applied
    _same_run(r, ref, [1e-3] + [o["deltaH"] for o in ref[:-1]], N)


@pytest.mark.parametrize("noise", ["gaussian", "contaminated"])
def test_small_n_runs_deferred_and_the_reference_order_stops_at_the_guard(tmp_path, noise):
    """the 300 x 60 case of test_robust_cpu.py::test_small_n_breakdown_when_no_residual_falls_inside_the_threshold"""
    N, M = 300, 60
    bed, D, beta, y = rs.case(N, M, 8, 9, noise)
    kw = dict(iterations=8, CG_max_iter=30, rho=0.5, seed=4, gam1=1e-8, stop_criteria_thr=1e-12)
    r = _run(bed, N, M, y, [0.7, 0.3], [0.0, 0.09], **kw)
    assert r.niter == 8
    for t in r.trace:
        assert all(np.isfinite(t[f]) for f in SCALARS + ("deltaH",)) and t["beta1"] < 1.0, t
    assert np.all(np.isfinite(r.x_est)) and np.corrcoef(r.x_est, beta)[0, 1] > 0.9

    pre = str(tmp_path / "ref")
    with pytest.raises(capi.GvError, match=r"stopped in iteration 2: 1 - beta1 is not strictly positive") as e:
        _run(bed, N, M, y, [0.7, 0.3], [0.0, 0.09], huber_delta_schedule="reference", out_prefix=pre, **kw)
    assert re.search(r"deltaH = [0-9.e+-]+, tau1 = [0-9.e+-]+, beta1 = 1\b", str(e.value)), str(e.value)
    for k in (1, 2):
        for name in ("_robust_it_%d.bin", "_robust_r1_it_%d.bin"):
            v = np.fromfile(pre + name % k)
            assert v.size == M and np.all(np.isfinite(v)), name % k
    assert not os.path.exists(pre + "_robust_it_3.bin")


def test_go_no_go_against_linear():
    """N = 4 000, M = 8 000, h2 = 0.5, 5 % causal markers: robust must not lose to linear on Gaussian noise and must beat it on
    noise of which 10 % is scaled by 10"""
    N, M, h2, frac = 4000, 8000, 0.5, 0.05
    rng = np.random.default_rng(41)
    beta = rng.standard_normal(M) * (rng.random(M) < frac) * np.sqrt(h2 / (frac * M))
    e = rng.standard_normal(N) * np.sqrt(1 - h2)
    cont = np.where(rng.random(N) < 0.1, 10.0, 1.0)
    probs, vars_ = [1 - frac, frac], [0.0, h2 / (frac * M)]
    kw = dict(iterations=8, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, stop_criteria_thr=1e-12, fuse_solves=4)
    corr = {}
    with capi.Shard(N, M) as sh:
        sh.upload_bed(synth.synth_bed(N, M, seed=41, miss_ppm=5000))
        sh.compute_markers_statistics()
        g = sh.Ax(beta * np.sqrt(N))[:N]
        for noise, eps in (("gaussian", e), ("contaminated", e * cont)):
            for model in ("linear", "robust"):
                r = hostapi.infere_linear(sh, g + eps, probs, vars_, model=model, gamw=2.0, history=False, **kw)
                assert r.niter == 8
                corr[noise, model] = np.corrcoef(r.x_est, beta)[0, 1]
    print("go/no-go corr(x, beta):", {"%s %s" % k: round(v, 4) for k, v in corr.items()})
    assert corr["gaussian", "robust"] >= corr["gaussian", "linear"] - 0.02, corr
    assert corr["contaminated", "robust"] >= corr["contaminated", "linear"] + 0.3, corr


def test_robust_forced_multi():
    N, M = 1001, 1500
    with _shard(N, M, 1, seed=11, miss_ppm=5000) as sh:
        rng = np.random.default_rng(11)
        beta = rng.standard_normal(M) * (rng.random(M) < 0.05) * 0.2
        e = rng.standard_normal(N) * np.where(rng.random(N) < 0.1, 10.0, 1.0)
        y = sh.Ax(beta * np.sqrt(N))[:N] + np.sqrt(0.5) * e
        kw = dict(iterations=5, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, model="robust", fuse_solves=4)

        def run():
            r = hostapi.infere_linear(sh, y, PROBS, VARS, **kw)
            t = _trace(r)
            t["z"] = [[float(s[k]) for k in ("beta1", "tau2", "tau1_next", "deltaH")] for s in r.trace]
            return t

        _check_all(sh, run)


def test_robust_on_dense_copy_matches_bed_run():
    N, M = 1001, 1500
    bed, X = _bed_case(N, M, 11)
    rng = np.random.default_rng(12)
    beta = rng.standard_normal(M) * (rng.random(M) < 0.05) * 0.2
    kw = dict(iterations=5, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, model="robust")
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        sb.compute_markers_statistics()
        y = sb.Ax(beta * np.sqrt(N))[:N] + np.sqrt(0.5) * rng.standard_normal(N) * np.where(rng.random(N) < 0.1, 10.0, 1.0)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, **kw)
    with capi.Shard(N, M) as sm:
        sm.upload_meth(X)
        rm = hostapi.infere_linear(sm, y, PROBS, VARS, **kw)
    assert rm.niter == rb.niter == 5
    assert [t["deltaH"] for t in rm.trace] == [t["deltaH"] for t in rb.trace]
    assert rel(rm.x_est, rb.x_est) < 1e-9


# ---- the driver --------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sharded(n, args):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_sharded.py"), "-n", str(n), "--comm", "host", "--same-gpu",
           "--master-port", str(_free_port()), "--", REAL] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_gvamp_main_real_robust_infere_shards_and_test_mode(tmp_path):
    N, M, iters = 1001, 1500, 4
    bed, D, beta, y = rs.case(N, M, 21, 22, "contaminated", **SPARSE)
    bedp, phen = str(tmp_path / "r.bed"), str(tmp_path / "r.phen")
    synth.write_bed(bedp, bed)
    with open(phen, "w") as f:
        for i in range(N):
            f.write("F%d I%d %.17g\n" % (i, i, y[i]))
    common = ["--run-mode", "infere", "--model", "robust", "--bed-file", bedp, "--phen-files", phen, "--N", N, "--Mt", M,
              "--iterations", iters, "--probs", "0.95,0.05", "--vars", "0,0.04", "--rho", "0.5", "--CG-max-iter", "30", "--seed", "3"]
    out1, out2 = str(tmp_path / "o1") + "/", str(tmp_path / "o2") + "/"
    _sharded(1, common + ["--out-dir", out1, "--out-name", "r"])
    _sharded(2, common + ["--out-dir", out2, "--out-name", "r"])
    # the hostapi run on the phenotype as the driver reads it: scaled, not centred (data.cpp:128-192), gam1 = 1e-6 (main_real.cpp:64)
    ys = y / np.sqrt(((y - y.mean()) ** 2).sum() / (N - 1))
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        r = hostapi.infere_linear(sh, ys, [0.95, 0.05], [0.0, 0.04], iterations=iters, CG_max_iter=30, rho=0.5, seed=3,
                                  gam1=1e-6, model="robust", fuse_solves=4)
    assert r.niter == iters
    # two shards draw their Onsager probe slice by slice (seed + S, vamp.cpp:875), so from iteration 2 on they follow another
    # sequence than one shard: they are held against the restatement with the same sliced probe
    two_ref = rs.robust_run(D, ys, [0.95, 0.05], [0.0, 0.04], iterations=iters, gam1=1e-6, rho=0.5, CG_max_iter=30, seed=3,
                            stop_criteria_thr=1e-4, shards=2)
    assert len(two_ref) == iters
    for k in range(1, iters + 1):
        for name, hist, key in (("r_robust_it_%d.bin", r.x1, "x1"), ("r_robust_r1_it_%d.bin", r.r1, "r1")):
            one, two = np.fromfile(out1 + name % k), np.fromfile(out2 + name % k)
            assert one.size == two.size == M
            assert rel(one, hist[k - 1]) < 1e-9, (name % k, rel(one, hist[k - 1]))
            assert rel(two, two_ref[k - 1][key] / np.sqrt(N)) < 1e-7, (name % k, rel(two, two_ref[k - 1][key] / np.sqrt(N)))
    assert rel(np.fromfile(out1 + "r_robust_it_1.bin"), np.fromfile(out2 + "r_robust_it_1.bin")) < 1e-9
    # --run-mode test reads the last iterate back through --estimate-file (main_real.cpp:183-211)
    est = out1 + "r_robust_it_%d.bin" % iters
    res = subprocess.run([REAL, "--run-mode", "test", "--bed-file-test", bedp, "--phen-files-test", phen, "--N-test", str(N),
                          "--Mt-test", str(M), "--estimate-file", est], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    z = D.Ax(np.fromfile(est) * np.sqrt(N))
    sd2 = ((ys - ys.mean()) ** 2).sum() / (N - 1)
    want = 1 - ((ys - z) ** 2).sum() / (sd2 * N)
    got = float(re.search(r"test R2 = ([-0-9.e+]+)", res.stdout).group(1))
    assert np.isclose(got, want, rtol=1e-5), (got, want)


def test_hostapi_refuses_unknown_model_and_schedule():
    N, M = 400, 300
    y = np.random.default_rng(0).standard_normal(N)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(synth.synth_bed(N, M, seed=2))
        with pytest.raises(capi.GvError, match="unknown huber_delta_schedule"):
            hostapi.infere_linear(sh, y, PROBS, VARS, model="robust", huber_delta_schedule="later")
        with pytest.raises(capi.GvError, match="unknown model"):
            hostapi.infere_linear(sh, y, PROBS, VARS, model="huber")
