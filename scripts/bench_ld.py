"""Two epilogues of one kernel, k_ld_block: the LD-score pass (gv_ld_scores) against the preconditioner's Gram
build (gvp::gram, section 13; gv_precond_info.build_seconds) on gv_synth_bed_ld genotypes, in one process.  Seconds and useful integer
MAC/s of both -- 4 products x N x the (j, k) entries delivered (the in-band entries of the scores, the clipped window squares of the
Grams); ratio_to_gram is the scores' rate over the Gram build's, i.e. how much of a block each epilogue delivers.  Writes one JSON file.

    python scripts/bench_ld.py --N 400000 --M 125000 --out profiles/ld_bench_400k_125k.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi  # noqa: E402


def gram_entries(M, W):
    """entries of the window Grams of both grids over the shard [0, M): sum of the clipped window lengths squared"""
    h = W // 2
    return sum((min((u + 1) * h, M) - max((u - 1) * h, 0)) ** 2 for u in range(0, (M - 1) // h + 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--ld-block", type=int, default=64)
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 512, 2048])
    ap.add_argument("--gram-window", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rounds = []
    with capi.Shard(a.N, a.M) as sh:
        sh.synth_bed(77, 5000, ld_block=a.ld_block, ld_ppm=900000)
        sh.compute_markers_statistics()
        for rd in range(a.rounds):
            row = {"round": rd}
            sh.set_cg_precond("scalar", a.gram_window)        # drops the Grams: the next read builds them again
            sh.set_cg_precond("ld", a.gram_window)
            sh.precond_window_gram(0, 0)
            secs = sh.precond_info()["build_seconds"]
            macs = 4.0 * a.N * gram_entries(a.M, a.gram_window)
            row["gram"] = dict(window=a.gram_window, seconds=secs, useful_macs=macs, macs_per_s=macs / secs)
            sh.set_cg_precond("scalar", a.gram_window)
            row["ld"] = []
            for B in a.windows:
                sh.ld_scores(B)
                st = sh.ld_info()
                row["ld"].append(dict(window=B, seconds=st["seconds"], useful_macs=st["useful_macs"], macs_per_s=st["useful_macs"] / st["seconds"],
                                      block_pairs=st["block_pairs"], scratch_bytes=st["scratch_bytes"],
                                      ratio_to_gram=st["useful_macs"] / st["seconds"] / row["gram"]["macs_per_s"]))
            rounds.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(N=a.N, M=a.M, ld_block=a.ld_block, layout="default", rounds=rounds), f)
        f.write("\n")


if __name__ == "__main__":
    main()
