"""gv_grm_he beside gv_grm_pairs on gv_synth_bed genotypes under the tile layout: a warm-up and --rounds rounds in
one process, each round timing three calls by the host clock of the whole call -- gv_grm_pairs at the cutoff (its kernel is the
yardstick: the K loop is the same, the epilogue a compare), gv_grm_he with 1 trait and gv_grm_he with 10 traits (standard normal
phenotypes, 2 % missing).  Per round: the seconds, the passes and blocks gv_grm_info reports, and the ratio to gv_grm_pairs.
Writes one JSON file.

    python scripts/bench_grm_he.py --N 50000 --M 125000 --out profiles/grm_he_50k_125k.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--cutoff", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((a.N, 10))
    Y[rng.random((a.N, 10)) < 0.02] = np.nan
    rows = []
    with capi.Shard(a.N, a.M) as sh:
        sh.set_layout(False, 2)
        sh.synth_bed(77, 5000)
        for rd in range(-1, a.rounds):          # (round -1 warms up and is not recorded)
            row = dict(round=rd)
            row["pairs_seconds"], got = timed(lambda: sh.grm_pairs(a.cutoff))
            row["pairs_found"] = int(len(got[0]))
            for tag, cols in (("he1", 1), ("he10", 10)):
                row[tag + "_seconds"], res = timed(lambda: sh.grm_he(Y[:, :cols]))
                st = sh.grm_info()
                row.update({tag + "_passes": st["passes"], tag + "_blocks_computed": st["blocks_computed"],
                            tag + "_block_pairs": st["block_pairs"], tag + "_scratch_bytes": st["scratch_bytes"],
                            tag + "_library_seconds": st["seconds"], tag + "_over_pairs": row[tag + "_seconds"] / row["pairs_seconds"]})
                row[tag + "_h2"] = [float(x) for x in res["h2"]]
                row[tag + "_se_jack"] = [float(x) for x in res["se_jack"]]
            if rd < 0:
                continue
            rows.append(row)
            print(json.dumps(row), flush=True)

    def med(key):
        v = sorted(r[key] for r in rows)
        return v[len(v) // 2]

    with open(a.out, "w") as f:
        json.dump(dict(N=a.N, M=a.M, cutoff=a.cutoff, layout="tile", pairs_seconds_median=med("pairs_seconds"),
                       he1_seconds_median=med("he1_seconds"), he10_seconds_median=med("he10_seconds"),
                       he1_over_pairs_median=med("he1_over_pairs"), he10_over_pairs_median=med("he10_over_pairs"), rounds=rows), f)
        f.write("\n")


if __name__ == "__main__":
    main()
