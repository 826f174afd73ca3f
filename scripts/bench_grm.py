"""gv_grm_pairs on gv_synth_bed genotypes under the tile layout: every pair of N individuals decided at a cutoff
over M markers, --rounds timed calls in one process after a warm-up.  Per round: the seconds of the call (gv_grm_info, the pre-pass
included), useful MAC/s = counting markers x N (N - 1) / 2 pairs per second, and computed fp64 MAC/s = 4096 x block pairs x the markers
padded to whole row groups per second (what the fp64 MFMAs multiplied, the diagonal blocks' lower halves and the pad rows included;
the one i8 product of the count plane is not in it).  The yardstick is the bare-loop rate of scripts/probes/mfma_f64_rate.hip
(--probe, its JSON line in a file).  Writes one JSON file.

    python scripts/bench_grm.py --N 50000 --M 125000 --probe profiles/mfma_f64_rate.json --out profiles/grm_50k_125k.json
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
    ap.add_argument("--cutoff", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe", default=None)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    probe = None
    if a.probe and os.path.exists(a.probe):
        with open(a.probe) as f:
            probe = json.load(f)
    rows = []
    with capi.Shard(a.N, a.M) as sh:
        sh.set_layout(False, 2)
        sh.synth_bed(77, 5000)
        kpad = (a.M + 63) // 64 * 64
        for rd in range(-1, a.rounds):          # (round -1 warms up and is not recorded)
            i, j, v, mc, d, dm = sh.grm_pairs(a.cutoff)
            st = sh.grm_info()
            if rd < 0:
                continue
            computed = 4096.0 * st["block_pairs"] * kpad
            row = dict(round=rd, seconds=st["seconds"], pairs_found=int(len(i)), block_pairs=st["block_pairs"],
                       counting_markers=st["counting_markers"], dropped_markers=st["dropped_markers"], useful_macs=st["useful_macs"],
                       useful_macs_per_s=st["useful_macs"] / st["seconds"], computed_f64_macs_per_s=computed / st["seconds"],
                       scratch_bytes=st["scratch_bytes"])
            if probe:
                best = max(probe["macs_per_s_1_wave_per_simd"], probe["macs_per_s_2_waves_per_simd"])
                row["computed_over_probe"] = row["computed_f64_macs_per_s"] / best
            rows.append(row)
            print(json.dumps(rows[-1]), flush=True)
    secs = sorted(r["seconds"] for r in rows)
    with open(a.out, "w") as f:
        json.dump(dict(N=a.N, M=a.M, cutoff=a.cutoff, layout="tile", seconds_median=secs[len(secs) // 2], probe=probe, rounds=rows), f)
        f.write("\n")


if __name__ == "__main__":
    main()
