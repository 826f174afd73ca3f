"""Scalar against LD-block preconditioned CG (DESIGN.md sections 13 and 18) on gv_synth_bed_ld genotypes (--kind bed) or on
gv_synth_dosage_ld's 8-bit dosage codes under gv_set_ld_dosage (--kind dosage8): VAMP iterations/s over iterations 2 onward at
--fuse-solves 4, passes, CG and Onsager steps per iteration, the Gram build, resident bytes.  The variants (scalar, ld at every window)
alternate on the same resident data in one process, --rounds times over; the first round of a data set also warms every shape up.
Writes one JSON file: every round's row, and per variant the median it/s and its spread (largest deviation of a round from the median).

    python scripts/bench_precond.py --N 400000 --M 125000 --ld-block 64 --iterations 5 --out profiles/precond_bench_400k_125k.json
    python scripts/bench_precond.py --kind dosage8 --N 20000 --M 800000 --ld-block 64 0 --rounds 3 \\
        --out profiles/precond_dosage_bench_20000x800000.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi, hostapi  # noqa: E402

PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]


def dosage_phen(sh, seed=9):
    """y = A beta + noise at h2 = 0.5, M / 50 causal markers, scaled as data::read_phen scales a phenotype"""
    rng = np.random.default_rng(seed)
    N, M = sh.N, sh.M
    beta = np.zeros(M)
    cv = rng.choice(M, size=max(1, M // 50), replace=False)
    beta[cv] = rng.standard_normal(cv.size) * np.sqrt(0.5 / cv.size)
    sh.compute_markers_statistics()
    g = sh.Ax(beta * np.sqrt(N))[:N]
    raw = g + np.std(g) * rng.standard_normal(N)
    return beta, raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["bed", "dosage8"], default="bed")
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--ld-block", type=int, nargs="+", default=[64, 48, 0])
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rows, summary = [], []
    for blk in a.ld_block:
        with capi.Shard(a.N, a.M) as sh:
            if a.kind == "bed":
                sh.synth_bed(77, 5000, ld_block=blk, ld_ppm=900000 if blk else 0)
                beta, y = hostapi.sim_phen(sh, 0.5, max(1, a.M // 50), 9)
            else:       # (independent codes: no entry takes the latent draw)
                sh.synth_dosage_ld(77, 8, blk if blk else 1, 900000 if blk else 0)
                sh.set_ld_dosage(1)
                beta, y = dosage_phen(sh)
            variants = [("scalar", 128)] + [("ld", w) for w in a.windows]
            rates = {v: [] for v in variants}
            for rnd in range(a.rounds):
                for kind, W in variants:
                    kw = dict(iterations=a.iterations, CG_max_iter=400, rho=0.5, seed=9, gam1=1e-8, gamw=2.0, stop_criteria_thr=1e-12,
                              fuse_solves=4, history=False, cg_precond=kind, cg_precond_window=W)
                    t0 = time.perf_counter()
                    r = hostapi.infere_linear(sh, y, PROBS, VARS, true_signal=beta, **kw)
                    wall = time.perf_counter() - t0
                    info = sh.precond_info()
                    tail = r.trace[1:]
                    secs = sum(t["seconds"] for t in tail)
                    row = dict(data=a.kind, ld_block=blk, kind=kind, window=W if kind == "ld" else None, round=rnd, wall_seconds=wall,
                               it_per_s_from_2=len(tail) / secs if secs > 0 else None,
                               passes=[t["n_ax_pass"] + t["n_atx_pass"] for t in r.trace],
                               cg_iters=[t["cg_iters"] for t in r.trace], onsager_iters=[t["onsager_iters"] for t in r.trace],
                               seconds=[t["seconds"] for t in r.trace])
                    if kind == "ld":
                        row.update(gram_build_seconds=info["build_seconds"], resident_bytes=info["resident_bytes"],
                                   factorisations=info["factorisations"], fallback_windows=info["fallback_windows"])
                    if row["it_per_s_from_2"]:
                        rates[(kind, W)].append(row["it_per_s_from_2"])
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            for (kind, W), rs in rates.items():
                if rs:
                    med = statistics.median(rs)
                    summary.append(dict(data=a.kind, ld_block=blk, kind=kind, window=W if kind == "ld" else None, rounds=len(rs),
                                        median_it_per_s_from_2=med, spread=max(abs(x - med) for x in rs) / med))
                    print(json.dumps(summary[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(data=a.kind, N=a.N, M=a.M, iterations=a.iterations, fuse_solves=4, rounds=a.rounds, rows=rows, summary=summary), f)
        f.write("\n")


if __name__ == "__main__":
    main()
