"""--model robust against bin_class and linear at one mid-size shape (default: the 8-GPU shard shape N = 400k x M = 125k) at
--fuse-solves 4: iterations/s, passes over the shard per iteration, and the wall time of the robust z side per iteration.

The z side of one iteration (vamp::infere_robust) is gv_huber_denoise, one gv_huber_delta (two in iteration 2
of the deferred schedule), the axpby that forms p2 and the guard's inner product of p2, each with its read-back; it is timed here
in isolation on the same N, on the p1 / y of a robust run.  Prints one JSON line.
  python scripts/bench_robust.py [--N 400000] [--M 125000] [--iterations 8] [--reps 50]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gvamp_amd import capi, hostapi  # noqa: E402

GRID = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 0.2, 0.4, 0.6, 0.8, 1, 1.5, 2, 3]     # vamp_Huber.cpp:259


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    N, M = a.N, a.M
    out = {"N": N, "M": M, "fuse_solves": 4, "iterations": a.iterations, "models": {}}
    with capi.Shard(N, M) as sh:
        sh.set_expected_passes(a.iterations * 12 * 3)
        sh.synth_bed(4242, 5000)
        sh.compute_markers_statistics()
        beta, y = hostapi.sim_phen(sh, 0.5, max(1, M // 100), 1)
        ybin = (y > np.median(y)).astype(np.float64)
        kw = dict(iterations=a.iterations, CG_max_iter=50, rho=0.5, seed=1, gam1=1e-8, history=False, fuse_solves=4,
                  stop_criteria_thr=1e-30)
        hostapi.infere_linear(sh, y, None, None, **dict(kw, iterations=2))       # picks, clocks
        for model, yy in (("linear", y), ("bin_class", ybin), ("robust", y)):
            r = hostapi.infere_linear(sh, yy, None, None, model=model, **kw)
            t = np.array([x["seconds"] for x in r.trace[2:]])
            p = np.array([x["n_ax_pass"] + x["n_atx_pass"] for x in r.trace[2:]])
            out["models"][model] = {"iterations": r.niter, "it_per_s": float(1.0 / t.mean()), "ms_per_iteration": float(1e3 * t.mean()),
                                    "passes_per_iteration": float(p.mean()),
                                    "cg_steps": [int(x["cg_iters"]) for x in r.trace]}
            if model == "robust":
                out["models"][model]["deltaH"] = [float(x["deltaH"]) for x in r.trace]
        # the z side in isolation: p1 = a stand-in cavity mean, y the same phenotype
        rng = np.random.default_rng(0)
        npad = 4 * ((N + 3) // 4)
        p1h, yh = np.zeros(npad), np.zeros(npad)
        p1h[:N] = y[:N] + rng.standard_normal(N)
        yh[:N] = y[:N]
        p1, yv, z1, p2 = sh.vecN(p1h), sh.vecN(yh), sh.vecN(), sh.vecN()
        parts = {}
        for name, fn in (("huber_denoise", lambda: sh.huber_denoise(p1, yv, 0.8, 0.6, z1)),
                         ("huber_delta", lambda: sh.huber_delta(p1, yv, 0.8, GRID)),
                         ("p2_axpby_and_guard_dot", lambda: (sh.axpby(p2, 1.0 / 0.3, z1, -0.7 / 0.3, p1), sh.dot(p2, p2, sync=0)))):
            fn()
            sh.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            sh.synchronize()
            parts[name] = 1e3 * (time.perf_counter() - t0) / a.reps
    z_ms = sum(parts.values())
    rob = out["models"]["robust"]
    out["z_side_ms"] = {k: round(v, 4) for k, v in parts.items()}
    out["z_side_ms_per_iteration"] = round(z_ms, 4)
    out["z_side_ms_iteration_2_deferred"] = round(z_ms + parts["huber_delta"], 4)
    out["z_side_share_of_robust_iteration"] = round(z_ms / rob["ms_per_iteration"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
