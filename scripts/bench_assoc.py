"""The association pass of compact dosage data (gv_assoc_loo) on one GPU beside one ATx of the same kind: prints ONE JSON line and,
with --out, writes it to a file (profiles/assoc_bench_<shape>.json).

  python scripts/bench_assoc.py [--N 20000] [--M 800000] [--kinds u8,u16] [--reps 5] [--rounds 3] [--seed 2026] [--out FILE]

The codes are generated on the device (gv_synth_dosage).  A LOO call is timed on the host around the whole entry point -- residual,
its two sums, the marker pass with the test in its epilogue, the copy of four M-vectors to the host -- after a device synchronise;
ATx the same way on device handles (no host copy).  Both stream the matrix once: `x_atx` is the LOO time over the ATx time.  Times
are the median over the rounds of the mean over --reps calls; TB/s are algorithmic, N * M * bits / 8 bytes per pass."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi  # noqa: E402

BYTES = {"u8": 1, "u16": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--M", type=int, default=800000)
    ap.add_argument("--kinds", default="u8,u16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, M = a.N, a.M
    kinds = [k for k in a.kinds.split(",") if k]
    assert kinds and all(k in BYTES for k in kinds), a.kinds
    rng = np.random.default_rng(a.seed)
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.01)
    res = {"metric": "dosage_assoc_loo", "N": N, "M": M, "reps": a.reps, "rounds": a.rounds, "kinds": {}}
    for k in kinds:
        with capi.Shard(N, M) as sh:
            sh.synth_dosage(a.seed, 8 * BYTES[k])
            sh.compute_markers_statistics()
            dx, dz, dw = sh.vecM(x1), sh.vecN(), sh.vecM()
            sh.ax_dev(dx, dz)
            y = dz.download()
            y[:N] += rng.standard_normal(N)
            dy = sh.vecN(y)
            t_loo, t_atx = [], []
            sh.assoc_calc(dz, dy, dx)            # warm-up
            sh.atx_dev(dy, dw)
            sh.synchronize()
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    out = sh.assoc_calc(dz, dy, dx)
                t_loo.append((time.perf_counter() - t0) / a.reps)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    sh.atx_dev(dy, dw)
                sh.synchronize()
                t_atx.append((time.perf_counter() - t0) / a.reps)
            loo, atx = float(np.median(t_loo)), float(np.median(t_atx))
            nbytes = N * M * BYTES[k]
            res["kinds"][k] = {"loo_ms": loo * 1e3, "atx_ms": atx * 1e3, "x_atx": loo / atx, "loo_TBs": nbytes / loo / 1e12,
                               "atx_TBs": nbytes / atx / 1e12, "min_p": float(np.nanmin(out["p"]))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
