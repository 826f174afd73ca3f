"""Compact dense data (8- / 16-bit dosage codes) products on one GPU, beside the dense fp64 kernels at the same shape: prints ONE
JSON line and, with --out, writes it to a file (profiles/dosage_bench_<shape>.json).

  python scripts/bench_dosage.py [--N 20000] [--M 800000] [--kinds u8,u16,f64,u8_mfma] [--reps 10] [--rounds 3] [--seed 2026] [--out FILE]
                                 [--miss-ppm P]

Every kind asked for is resident at once (one context each; u8 + u16 + f64 at 20 000 x 800 000 are 16 + 32 + 128 GB) and the timed
rounds alternate between them in one process: round r times Ax, ATx and both two-vector forms of every kind before round r + 1
starts, so a drift of the box touches all kinds alike.  The codes are generated on the device (gv_synth_dosage).  The fp64 matrix
holds scale * B -- the same values -- when the shape is small enough to convert on the host (N * M <= 2e8); above that it is the
device-generated gv_synth_meth matrix of the same shape: these kernels stream every entry whatever it holds, so their time does not
depend on the values.  Times are HIP events around each whole product (gv_set_timing 1: the streaming kernel plus, for Ax, its
segment reduction), the median over the rounds of the mean over --reps calls.  TB/s are algorithmic: N * M * bits / 8 bytes of matrix
per pass (the padding and the vectors not counted); `share` is against 8 TB/s; `x_f64` is the fp64 pass time over this kind's.
--kinds u8 alone serves the GWAS-shaped run (N 200 000 x M 500 000, 100 GB).

--miss-ppm P (missing entries, gv_set_dosage_missing): every code kind k runs twice in the same alternation -- `k`, the plain kernels,
on gv_synth_dosage_na(seed, bits, 0) in a context that takes the shortcut (no reserved code counted), and `k_na`, the missing-aware
kernels forced by GV_DOSAGE_NA_KERNELS=1, on gv_synth_dosage_na(seed, bits, P).  With P = 0 the two hold the same codes, read the same
bytes and give the same bits, so `<product>_x_plain` = time(k_na) / time(k) is the cost of the compare and select alone.

Kind u8_mfma: the codes of u8 in a context of its own on the fixed-point i8 MFMA route (gv_set_dosage_route(ctx, 1)), timed in the same
alternation; with u8 among the kinds `<product>_x_u8` = time(u8) / time(u8_mfma) -- above 1 the route is faster -- and
`<product>_spread` the largest relative deviation of a round from the median over both kinds, the resolution of that ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvamp_amd import capi, synth  # noqa: E402

PEAK_TBS = 8.0
BYTES = {"u8": 1, "u16": 2, "f64": 8, "u8_mfma": 1}
BITS = {"u8": 8, "u16": 16, "u8_mfma": 8}
PRODUCTS = ("Ax", "ATx", "Ax2", "ATx2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--M", type=int, default=800000)
    ap.add_argument("--kinds", default="u8,u16,f64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    ap.add_argument("--miss-ppm", type=int, default=None)
    a = ap.parse_args()
    N, M = a.N, a.M
    kinds = [k for k in a.kinds.split(",") if k]
    assert kinds and all(k in BYTES for k in kinds), a.kinds
    if a.miss_ppm is not None:
        kinds = [kk for k in kinds for kk in ((k, k + "_na") if k in ("u8", "u16") else (k,))]
        for k in ("u8", "u16"):
            BYTES[k + "_na"], BITS[k + "_na"] = BYTES[k], BITS[k]
    rng = np.random.default_rng(a.seed)
    xs = [rng.standard_normal(M), rng.standard_normal(M)]
    res = {"metric": "dosage_products", "N": N, "M": M, "reps": a.reps, "rounds": a.rounds, "peak_TBs": PEAK_TBS, "kinds": {}}
    same_values = N * M <= 2e8
    res["f64_values"] = "scale * codes (u8)" if same_values else "gv_synth_meth (same shape)"
    if a.miss_ppm is not None:
        res["miss_ppm"] = a.miss_ppm
    shards, run = {}, {}
    try:
        for k in kinds:
            if k.endswith("_na"):                  # read by gv_create, per context
                os.environ["GV_DOSAGE_NA_KERNELS"] = "1"
            else:
                os.environ.pop("GV_DOSAGE_NA_KERNELS", None)
            sh = capi.Shard(N, M)
            shards[k] = sh
            if k == "u8_mfma":
                sh.set_dosage_route(1)
            t0 = time.perf_counter()
            if k == "f64" and same_values:
                sh.upload_meth(synth.synth_dosage(N, M, a.seed, 8).astype(np.float64) / 127.0)
            elif k == "f64":
                sh.synth_meth(a.seed)
            elif a.miss_ppm is not None:
                sh.synth_dosage_na(a.seed, BITS[k], a.miss_ppm if k.endswith("_na") else 0)
            else:
                sh.synth_dosage(a.seed, BITS[k])
            ingest = time.perf_counter() - t0
            t0 = time.perf_counter()
            sh.compute_markers_statistics()
            info = {"matrix_GB": N * M * BYTES[k] / 1e9, "ingest_s": ingest, "stats_ms": (time.perf_counter() - t0) * 1e3,
                    "layout": sh.get_layout()}
            if k != "f64":
                info["dosage_info"] = sh.dosage_info()
                info["dosage_route"] = list(sh.dosage_route())
                assert info["dosage_route"][1] == (1 if k == "u8_mfma" else 0), (k, info["dosage_route"])
            res["kinds"][k] = info
            x, x2 = sh.vecM(xs[0]), sh.vecM(xs[1])
            pn = np.zeros(4 * sh.mbytes)
            pn[:N] = rng.standard_normal(N)
            p, p2 = sh.vecN(pn), sh.vecN(pn[::-1].copy())
            z, z2, w, w2 = sh.vecN(), sh.vecN(), sh.vecM(), sh.vecM()
            run[k] = {"Ax": lambda sh=sh, x=x, z=z: sh.ax_dev(x, z), "ATx": lambda sh=sh, p=p, w=w: sh.atx_dev(p, w),
                      "Ax2": lambda sh=sh, x=x, x2=x2, z=z, z2=z2: sh.ax2_dev(x, x2, z, z2),
                      "ATx2": lambda sh=sh, p=p, p2=p2, w=w, w2=w2: sh.atx2_dev(p, p2, w, w2)}
            for fn in run[k].values():          # warm-up (the first Ax allocates its partial vectors)
                fn()
            sh.synchronize()
        times = {k: {pr: [] for pr in PRODUCTS} for k in kinds}
        for _ in range(a.rounds):
            for pr in PRODUCTS:
                for k in kinds:                 # the kinds alternate inside every round
                    sh = shards[k]
                    sh.set_timing(1)
                    sh.counters(reset=True)
                    for _ in range(a.reps):
                        run[k][pr]()
                    c = sh.counters(reset=True)
                    sh.set_timing(0)
                    times[k][pr].append((c["ms_ax"] + c["ms_atx"]) / a.reps)
        for k in kinds:
            for pr in PRODUCTS:
                ms = float(np.median(times[k][pr]))
                d = res["kinds"][k]
                d[pr + "_ms"] = ms
                d[pr + "_ms_rounds"] = times[k][pr]
                d[pr + "_TBs"] = N * M * BYTES[k] / (ms * 1e-3) / 1e12
                d[pr + "_share"] = d[pr + "_TBs"] / PEAK_TBS
                d[pr + "_Tentries_s"] = N * M / (ms * 1e-3) / 1e12
        if "f64" in kinds:
            for k in kinds:
                for pr in PRODUCTS:
                    res["kinds"][k][pr + "_x_f64"] = res["kinds"]["f64"][pr + "_ms"] / res["kinds"][k][pr + "_ms"]
        if "u8_mfma" in kinds and "u8" in kinds:
            for pr in PRODUCTS:
                d = res["kinds"]["u8_mfma"]
                d[pr + "_x_u8"] = res["kinds"]["u8"][pr + "_ms"] / d[pr + "_ms"]
                d[pr + "_spread"] = max(abs(t - res["kinds"][k][pr + "_ms"]) / res["kinds"][k][pr + "_ms"]
                                        for k in ("u8", "u8_mfma") for t in times[k][pr])
        for k in kinds:
            if k.endswith("_na"):
                for pr in PRODUCTS:
                    res["kinds"][k][pr + "_x_plain"] = res["kinds"][k][pr + "_ms"] / res["kinds"][k[:-3]][pr + "_ms"]
    finally:
        for sh in shards.values():
            sh.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
