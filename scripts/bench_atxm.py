#!/usr/bin/env python3
"""gv_atxm_dev against what the library offered before it for the same batch, on one synthetic shard.

For C in {2, 4, 8, 16, 32} and each GV_ATXM_COLS in {4, 8}, in ONE process, after a warm-up, in at least three alternating rounds:
  (a) gv_atxm_dev on its kernel (GV_ATXM_KERNEL=1 so that every C takes it);
  (b) ceil(C / 2) gv_atx2_dev calls, plus one gv_atx_dev for an odd C, on the same context.
Each leg is a host clock around `reps` back-to-back batches that end in a device synchronise, reps chosen so that a window is at
least --window seconds.  Once per leg (a) and (b) are compared bit for bit.  Every round goes to the JSON file, not a mean alone;
`ratio` = median(b) / median(a), `spread` = the relative range of the leg's own per-round ratios.

    python scripts/bench_atxm.py                        # N = 400 000 x M = 125 000, writes profiles/atxm_400k_125k.json
    python scripts/bench_atxm.py --N 400000 --M 1000000 --out profiles/atxm_400k_1m.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of device work per timed window")
    ap.add_argument("--counts", default="2,4,8,16,32")
    ap.add_argument("--cols", default="4,8")
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 3
    from gvamp_amd import capi
    counts = [int(t) for t in a.counts.split(",")]
    cols = [int(t) for t in a.cols.split(",")]
    cmax = max(counts)
    out = a.out or os.path.join(ROOT, "profiles", "atxm_%dk_%dk.json" % (a.N // 1000, a.M // 1000))
    os.environ["GV_ATXM_KERNEL"] = "1"
    os.environ.pop("GV_ATXM_KS", None)
    rng = np.random.default_rng(a.seed)
    npad = 4 * ((a.N + 3) // 4)
    Y = []
    for _ in range(cmax):
        y = np.zeros(npad)
        y[:a.N] = rng.standard_normal(a.N) * 10.0 ** rng.integers(-3, 4)
        Y.append(y)
    legs = []
    for cp in cols:
        os.environ["GV_ATXM_COLS"] = str(cp)
        sh = capi.Shard(a.N, a.M)
        sh.set_layout(False, 2)
        sh.synth_bed(a.seed, 5000)
        sh.compute_markers_statistics()
        xs = [sh.vecN(y) for y in Y]
        za, zb = [sh.vecM() for _ in range(cmax)], [sh.vecM() for _ in range(cmax)]

        def new(C):
            sh.atxm_dev(xs[:C], za[:C])

        def old(C):
            j = 0
            while j + 2 <= C:
                sh.atx2_dev(xs[j], xs[j + 1], zb[j], zb[j + 1])
                j += 2
            if j < C:
                sh.atx_dev(xs[j], zb[j])

        def timed(fn, C, reps):
            sh.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn(C)
            sh.synchronize()
            return (time.perf_counter() - t0) / reps

        for C in counts:
            new(C)
            old(C)              # warm-up of both legs (the first gv_atx2_dev also makes the library's pick of its decompositions)
            info = sh.atxm_info()
            assert info["path"] == "kernel", info
            same = all(np.array_equal(za[j].download().view(np.uint64), zb[j].download().view(np.uint64)) for j in range(C))
            assert same, "gv_atxm_dev and the two-vector passes differ at C = %d, GV_ATXM_COLS = %d" % (C, cp)
            reps_a = max(1, int(a.window / max(timed(new, C, 1), 1e-6)) + 1)
            reps_b = max(1, int(a.window / max(timed(old, C, 1), 1e-6)) + 1)
            ra, rb = [], []
            for _ in range(a.rounds):
                ra.append(timed(new, C, reps_a))
                rb.append(timed(old, C, reps_b))
            ratios = [b / t for t, b in zip(ra, rb)]
            leg = dict(C=C, atxm_cols=cp, cols_per_pass=info["cols_per_pass"], passes=info["passes"], ksegs=info["ksegs"],
                       scratch_bytes=info["scratch_bytes"], bit_identical=bool(same), reps_atxm=reps_a, reps_atx2=reps_b,
                       atxm_ms=[1e3 * t for t in ra], atx2_ms=[1e3 * t for t in rb],
                       ms_per_pass=float(1e3 * np.median(ra) / info["passes"]), ratio_rounds=ratios,
                       ratio=float(np.median(rb) / np.median(ra)), spread=float((max(ratios) - min(ratios)) / np.median(ratios)))
            legs.append(leg)
            print("C=%2d cols=%2d  atxm %8.3f ms  atx2 %8.3f ms  ratio %.3f  spread %.3f" %
                  (C, cp, 1e3 * np.median(ra), 1e3 * np.median(rb), leg["ratio"], leg["spread"]), flush=True)
        for v in xs + za + zb:
            v.free()
        sh.close()
    res = dict(what="gv_atxm_dev (a) against ceil(C/2) gv_atx2_dev passes (b) on one context; ratio = b / a", N=a.N, M=a.M,
               rounds=a.rounds, window_s=a.window, seed=a.seed, legs=legs)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=os.path.relpath(out, ROOT), legs=len(legs))))


if __name__ == "__main__":
    main()
