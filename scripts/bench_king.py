"""gv_king_pairs on gv_synth_bed genotypes under the tile layout: every pair of N individuals decided at the
second-degree cutoff over M markers, --rounds timed calls in one process after a warm-up.  Per round: the seconds of the call
(gv_king_info), useful integer MAC/s = 5 products x M x N (N - 1) / 2 pairs per second, and computed MAC/s = 5 x 4096 x block pairs x
the markers padded to whole row groups per second (what the MFMAs multiplied, the diagonal blocks' lower halves and the pad rows
included).  The yardstick is the LD block kernel's rate in profiles/ld_gram_block_400k_125k.json.  Writes one JSON file.

    python scripts/bench_king.py --N 50000 --M 125000 --out profiles/king_50k_125k.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--cutoff", type=float, default=0.0884)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rows = []
    with capi.Shard(a.N, a.M) as sh:
        sh.set_layout(False, 2)
        sh.synth_bed(77, 5000)
        kpad = (a.M + 63) // 64 * 64
        for rd in range(-1, a.rounds):          # (round -1 warms up and is not recorded)
            i, j, kin, cnt = sh.king_pairs(a.cutoff)
            st = sh.king_info()
            if rd < 0:
                continue
            computed = 5.0 * 4096.0 * st["block_pairs"] * kpad
            rows.append(dict(round=rd, seconds=st["seconds"], pairs_found=int(len(i)), block_pairs=st["block_pairs"],
                             useful_macs=st["useful_macs"], useful_macs_per_s=st["useful_macs"] / st["seconds"],
                             computed_macs_per_s=computed / st["seconds"], scratch_bytes=st["scratch_bytes"]))
            print(json.dumps(rows[-1]), flush=True)
    secs = sorted(r["seconds"] for r in rows)
    with open(a.out, "w") as f:
        json.dump(dict(N=a.N, M=a.M, cutoff=a.cutoff, layout="tile", seconds_median=secs[len(secs) // 2], rounds=rows), f)
        f.write("\n")


if __name__ == "__main__":
    main()
