"""Methylation (dense fp64) products and VAMP on one GPU: prints ONE JSON line.

  python scripts/bench_meth.py [--N 20000] [--M 800000] [--reps 10] [--iterations 5] [--seed 2026]

The matrix is generated on the device (gv_synth_meth).  Ax, ATx and both two-vector forms are timed with HIP events around each
whole product (gv_set_timing 1: the streaming kernel plus, for Ax, its segment reduction); GB/s are algorithmic (M * N * 8 bytes
of matrix per pass, the padding not counted) and the roofline fraction is against 8 TB/s.  VAMP iterations/s come from a seeded
sparse effect vector and the drivers' default --fuse-solves level (4)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi, hostapi  # noqa: E402

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--M", type=int, default=800000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    N, M = a.N, a.M
    nbytes = 8.0 * N * M
    rng = np.random.default_rng(a.seed)
    res = {"metric": "meth_products", "N": N, "M": M, "matrix_GB": nbytes / 1e9, "peak_GBs": PEAK_GBS}
    with capi.Shard(N, M) as sh:
        t0 = time.perf_counter()
        sh.synth_meth(a.seed)
        res["synth_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        sh.compute_markers_statistics()
        res["stats_ms"] = (time.perf_counter() - t0) * 1e3
        x, x2 = sh.vecM(rng.standard_normal(M)), sh.vecM(rng.standard_normal(M))
        pn = np.zeros(4 * sh.mbytes)
        pn[:N] = rng.standard_normal(N)
        p, p2 = sh.vecN(pn), sh.vecN(pn[::-1].copy())
        z, z2, w, w2 = sh.vecN(), sh.vecN(), sh.vecM(), sh.vecM()
        cases = {"Ax": lambda: sh.ax_dev(x, z), "ATx": lambda: sh.atx_dev(p, w),
                 "Ax2": lambda: sh.ax2_dev(x, x2, z, z2), "ATx2": lambda: sh.atx2_dev(p, p2, w, w2)}
        for name, fn in cases.items():
            fn()                                   # warm-up (the first Ax allocates its partial vectors)
            sh.synchronize()
            sh.set_timing(1)
            sh.counters(reset=True)
            for _ in range(a.reps):
                fn()
            c = sh.counters(reset=True)
            sh.set_timing(0)
            ms = (c["ms_ax"] + c["ms_atx"]) / a.reps
            res[name + "_ms"] = ms
            res[name + "_GBs"] = nbytes / (ms * 1e-3) / 1e9
            res[name + "_roofline"] = res[name + "_GBs"] / PEAK_GBS
        res["Ax2_over_Ax"] = res["Ax2_ms"] / res["Ax_ms"]
        res["ATx2_over_ATx"] = res["ATx2_ms"] / res["ATx_ms"]
        beta = np.zeros(M)
        idx = rng.choice(M, max(1, M // 500), replace=False)
        beta[idx] = rng.standard_normal(idx.size) * np.sqrt(0.5 / idx.size)
        y = sh.Ax(beta * np.sqrt(N))[:N]
        y = y + rng.standard_normal(N) * np.std(y)
        t0 = time.perf_counter()
        r = hostapi.infere_linear(sh, y, [0.98, 0.02], [0.0, 1e-3], iterations=a.iterations, CG_max_iter=30, rho=0.5,
                                  seed=1, gam1=1e-6, gamw=1.0, history=False, fuse_solves=4)
        wall = time.perf_counter() - t0
        res["vamp_iterations"] = r.niter
        res["vamp_seconds"] = wall
        res["vamp_it_per_s"] = r.niter / wall
        res["vamp_cg_iters"] = [t["cg_iters"] for t in r.trace]
        res["vamp_passes"] = [t["n_ax_pass"] + t["n_atx_pass"] for t in r.trace]
        res["x_hat_finite"] = bool(np.all(np.isfinite(r.x_est)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
