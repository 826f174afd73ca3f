"""Scalar against LD-block preconditioned CG on gv_synth_bed_ld genotypes: VAMP iterations/s over iterations
2 onward at --fuse-solves 4, passes, CG and Onsager steps per iteration, the Gram build, resident bytes.  Writes one JSON file.

    python scripts/bench_precond.py --N 400000 --M 125000 --ld-block 64 --iterations 5 --out profiles/precond_bench_400k_125k.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi, hostapi  # noqa: E402

PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--ld-block", type=int, nargs="+", default=[64, 48, 0])
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rows = []
    for blk in a.ld_block:
        with capi.Shard(a.N, a.M) as sh:
            sh.synth_bed(77, 5000, ld_block=blk, ld_ppm=900000 if blk else 0)
            beta, y = hostapi.sim_phen(sh, 0.5, max(1, a.M // 50), 9)
            for kind, W in [("scalar", 128)] + [("ld", w) for w in a.windows]:
                kw = dict(iterations=a.iterations, CG_max_iter=400, rho=0.5, seed=9, gam1=1e-8, gamw=2.0, stop_criteria_thr=1e-12,
                          fuse_solves=4, history=False, cg_precond=kind, cg_precond_window=W)
                t0 = time.perf_counter()
                r = hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, **kw)
                wall = time.perf_counter() - t0
                info = sh.precond_info()
                tail = r.trace[1:]
                secs = sum(t["seconds"] for t in tail)
                row = dict(ld_block=blk, kind=kind, window=W if kind == "ld" else None, wall_seconds=wall,
                           it_per_s_from_2=len(tail) / secs if secs > 0 else None,
                           passes=[t["n_ax_pass"] + t["n_atx_pass"] for t in r.trace],
                           cg_iters=[t["cg_iters"] for t in r.trace], onsager_iters=[t["onsager_iters"] for t in r.trace],
                           seconds=[t["seconds"] for t in r.trace])
                if kind == "ld":
                    row.update(gram_build_seconds=info["build_seconds"], resident_bytes=info["resident_bytes"],
                               factorisations=info["factorisations"], fallback_windows=info["fallback_windows"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(N=a.N, M=a.M, iterations=a.iterations, fuse_solves=4, rows=rows), f)
        f.write("\n")


if __name__ == "__main__":
    main()
