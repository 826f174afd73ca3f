#!/usr/bin/env python3
"""The covariate-adjusted screen (gv_screen_cov_set / gv_screen_cov_dev) beside the marginal screen
(gv_screen_dev) on one synthetic shard, in ONE process after a warm-up.

  set    gv_screen_cov_set with K covariates (columns of standard normals, one of them turned into 55 +- 8 and one into 0 / 1): its
         seconds from the device events the library records, split into the batch product and the panel kernels, every round.
  call   for C in --counts: gv_screen_cov_dev (all five outputs) and gv_screen_dev (all three) on the same C raw / prepared columns, in
         alternating rounds.  Each leg is a host clock around `reps` back-to-back calls that end in a device synchronise (what
         scripts/bench_atxm.py does; gv_screen_dev records no events of its own), reps chosen so that a window is at least --window
         seconds; for gv_screen_cov_dev the library's own device-event split (product / panel and finishing kernels) is kept beside it.

`ratio` = median(cov) / median(marginal): what adjusting for K covariates costs per call once the set is cached.

    python scripts/bench_screen_cov.py                  # N = 400 000 x M = 125 000, K = 10, writes profiles/screen_cov_400k_125k.json
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
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of device work per timed window")
    ap.add_argument("--counts", default="8,64")
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 3
    from gvamp_amd import capi
    counts = [int(t) for t in a.counts.split(",")]
    cmax = max(counts)
    out = a.out or os.path.join(ROOT, "profiles", "screen_cov_%dk_%dk.json" % (a.N // 1000, a.M // 1000))
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL"):
        os.environ.pop(k, None)
    rng = np.random.default_rng(a.seed)
    Cov = rng.standard_normal((a.K, a.N))
    if a.K >= 2:
        Cov[0] = 55.0 + 8.0 * Cov[0]
        Cov[1] = (Cov[1] > 0.2).astype(np.float64)
    Y = rng.standard_normal((cmax, a.N)) * 10.0 ** rng.integers(-3, 4, size=(cmax, 1)) + rng.standard_normal((cmax, a.K)) @ Cov

    sh = capi.Shard(a.N, a.M)
    sh.set_layout(False, 2)
    sh.synth_bed(a.seed, 5000)
    sh.compute_markers_statistics()
    cv = [sh.vecN(sh._padN(c)) for c in Cov]
    ys = [sh.vecN(sh._padN(y)) for y in Y]
    us = [sh.vecN(u) for u in sh.screen_prepare(Y)]
    oc = [[sh.vecM() for _ in range(cmax)] for _ in range(5)]
    om = [[sh.vecM() for _ in range(cmax)] for _ in range(3)]

    sets = []
    for rnd in range(a.rounds + 1):                       # the first round is the warm-up (scratch and cache allocation)
        sh.screen_cov_set(cv)
        info = sh.screen_cov_info()
        if rnd:
            sets.append(dict(products_ms=1e3 * info["set_seconds_products"], panel_ms=1e3 * info["set_seconds_panel"],
                             wall_ms=1e3 * info["set_seconds"]))
    cached = info["cached_bytes"]
    print("set K=%d: products %.3f ms  panel kernels %.3f ms  wall %.3f ms  cached %.1f MB" %
          (a.K, np.median([s["products_ms"] for s in sets]), np.median([s["panel_ms"] for s in sets]),
           np.median([s["wall_ms"] for s in sets]), cached / 1e6), flush=True)

    def cov(C):
        sh.screen_cov_dev(ys[:C], *[o[:C] for o in oc])

    def marg(C):
        sh.screen_dev(us[:C], *[o[:C] for o in om])

    def timed(fn, C, reps):
        sh.synchronize()
        t0 = time.perf_counter()
        ev = [0.0, 0.0]
        for _ in range(reps):
            fn(C)
            if fn is cov:
                i = sh.screen_cov_info()
                ev[0] += i["call_seconds_products"]
                ev[1] += i["call_seconds_panel"]
        sh.synchronize()
        return (time.perf_counter() - t0) / reps, ev[0] / reps, ev[1] / reps

    legs = []
    for C in counts:
        cov(C)
        marg(C)
        path = sh.atxm_info()["path"]
        reps_a = max(1, int(a.window / max(timed(cov, C, 1)[0], 1e-6)) + 1)
        reps_b = max(1, int(a.window / max(timed(marg, C, 1)[0], 1e-6)) + 1)
        ra, rb = [], []
        for _ in range(a.rounds):
            ra.append(timed(cov, C, reps_a))
            rb.append(timed(marg, C, reps_b)[0])
        wall = [t[0] for t in ra]
        ratios = [t / b for t, b in zip(wall, rb)]
        leg = dict(C=C, K=a.K, path=path, reps_cov=reps_a, reps_marginal=reps_b, cov_ms=[1e3 * t for t in wall],
                   cov_products_ms=[1e3 * t[1] for t in ra], cov_panel_ms=[1e3 * t[2] for t in ra], marginal_ms=[1e3 * t for t in rb],
                   ratio_rounds=ratios, ratio=float(np.median(wall) / np.median(rb)),
                   panel_share=float(np.median([t[2] for t in ra]) / np.median([t[1] + t[2] for t in ra])),
                   spread=float((max(ratios) - min(ratios)) / np.median(ratios)))
        legs.append(leg)
        print("C=%2d K=%2d  cov %8.3f ms (products %8.3f, panel and finishing %7.3f: share %.3f)  marginal %8.3f ms  ratio %.3f  spread %.3f" %
              (C, a.K, 1e3 * np.median(wall), np.median(leg["cov_products_ms"]), np.median(leg["cov_panel_ms"]), leg["panel_share"],
               1e3 * np.median(rb), leg["ratio"], leg["spread"]), flush=True)
    sh.close()
    res = dict(what="gv_screen_cov_dev (five outputs, K covariates cached by gv_screen_cov_set) against gv_screen_dev (three outputs) on the "
                    "same C columns of one context; ratio = cov / marginal; *_products_ms / *_panel_ms are the library's device events",
               N=a.N, M=a.M, K=a.K, rounds=a.rounds, window_s=a.window, seed=a.seed, cached_bytes=cached, set=sets, legs=legs)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=os.path.relpath(out, ROOT), legs=len(legs))))


if __name__ == "__main__":
    main()
