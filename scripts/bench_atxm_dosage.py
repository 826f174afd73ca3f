#!/usr/bin/env python3
"""gv_atxm_dev on 8-bit dosage codes under the fixed-point route against what the library offered before it for the same batch, on one
synthetic shard, in the manner of scripts/bench_atxm.py.

For C in {2, 3, 4, 8, 16, 32}, each GV_ATXM_COLS in {4, 8} and each GV_ATXM_TILES asked for, in ONE process, one context on route 1 per
(cols, tiles), after a warm-up, in at least three alternating rounds:
  (a) gv_atxm_dev on its kernel (GV_ATXM_KERNEL=1 so that every C takes it);
  (b) ceil(C / 2) gv_atx2_dev calls, plus one gv_atx_dev for an odd C, on the same context -- what gv_atxm_dev ran before the kernel.
Each leg is a host clock around `reps` back-to-back batches that end in a device synchronise, reps chosen so that a window is at
least --window seconds.  Once per leg (a) and (b) are compared bit for bit.  Every round goes to the JSON file, not a mean alone;
`ratio` = median(b) / median(a), `spread` = the relative range of the leg's own per-round ratios.
For context only: the same C through gv_atxm_dev of a route-0 context (the fp64 VALU kernels, in pairs), and the split of
gv_screen_dev and gv_screen_cov_dev (K = 10) at C = 8 and 64 on route 1 between the product and the panel and finishing kernels.

    python scripts/bench_atxm_dosage.py          # N = 20 000 x M = 800 000, writes profiles/atxm_dosage8_20000x800000.json
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
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--M", type=int, default=800000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of device work per timed window")
    ap.add_argument("--counts", default="2,3,4,8,16,32")
    ap.add_argument("--cols", default="4,8")
    ap.add_argument("--tiles", default="0", help="GV_ATXM_TILES values, 0 = the library's pick")
    ap.add_argument("--screens", default="8,64", help="column counts of the screen split ('' = none)")
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 3
    from gvamp_amd import capi
    counts = [int(t) for t in a.counts.split(",")]
    cmax = max(counts)
    out = a.out or os.path.join(ROOT, "profiles", "atxm_dosage8_%dx%d.json" % (a.N, a.M))
    os.environ["GV_ATXM_KERNEL"] = "1"
    rng = np.random.default_rng(a.seed)
    npad = 4 * ((a.N + 3) // 4)
    Y = []
    for _ in range(cmax):
        y = np.zeros(npad)
        y[:a.N] = rng.standard_normal(a.N) * 10.0 ** rng.integers(-3, 4)
        Y.append(y)

    def shard(route):
        sh = capi.Shard(a.N, a.M)
        sh.set_dosage_route(route)
        sh.synth_dosage(a.seed, 8)
        m4 = np.full(sh.mbytes, 0x0F, dtype=np.uint8)          # every individual has a phenotype
        if a.N % 4:
            m4[-1] = (1 << (a.N % 4)) - 1
        sh.set_mask(m4, a.N)
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (route, route)
        return sh

    def timed(sh, fn, reps):
        sh.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sh.synchronize()
        return (time.perf_counter() - t0) / reps

    legs = []
    for cp in [int(t) for t in a.cols.split(",")]:
        for tiles in [int(t) for t in a.tiles.split(",")]:
            os.environ["GV_ATXM_COLS"] = str(cp)
            os.environ.pop("GV_ATXM_TILES", None)
            if tiles:
                os.environ["GV_ATXM_TILES"] = str(tiles)
            sh = shard(1)
            xs = [sh.vecN(y) for y in Y]
            za, zb = [sh.vecM() for _ in range(cmax)], [sh.vecM() for _ in range(cmax)]

            def old(C):
                j = 0
                while j + 2 <= C:
                    sh.atx2_dev(xs[j], xs[j + 1], zb[j], zb[j + 1])
                    j += 2
                if j < C:
                    sh.atx_dev(xs[j], zb[j])

            for C in counts:
                new_c, old_c = (lambda C=C: sh.atxm_dev(xs[:C], za[:C])), (lambda C=C: old(C))
                new_c()
                old_c()
                info = sh.atxm_info()
                assert info["path"] == "kernel", info
                same = all(np.array_equal(za[j].download().view(np.uint64), zb[j].download().view(np.uint64)) for j in range(C))
                assert same, "gv_atxm_dev and the two-vector passes differ at C = %d, GV_ATXM_COLS = %d" % (C, cp)
                reps_a = max(1, int(a.window / max(timed(sh, new_c, 1), 1e-6)) + 1)
                reps_b = max(1, int(a.window / max(timed(sh, old_c, 1), 1e-6)) + 1)
                ra, rb = [], []
                for _ in range(a.rounds):
                    ra.append(timed(sh, new_c, reps_a))
                    rb.append(timed(sh, old_c, reps_b))
                ratios = [b / t for t, b in zip(ra, rb)]
                leg = dict(C=C, atxm_cols=cp, tiles=tiles, cols_per_pass=info["cols_per_pass"], passes=info["passes"], ksegs=info["ksegs"],
                           scratch_bytes=info["scratch_bytes"], bit_identical=bool(same), reps_atxm=reps_a, reps_atx2=reps_b,
                           atxm_ms=[1e3 * t for t in ra], atx2_ms=[1e3 * t for t in rb],
                           ms_per_pass=float(1e3 * np.median(ra) / info["passes"]),
                           atx2_ms_per_pass=float(1e3 * np.median(rb) / -(-C // 2)), ratio_rounds=ratios,
                           ratio=float(np.median(rb) / np.median(ra)), spread=float((max(ratios) - min(ratios)) / np.median(ratios)))
                legs.append(leg)
                print("C=%2d cols=%d tiles=%d  atxm %8.3f ms (%6.3f / pass)  atx2 %8.3f ms (%6.3f / pass)  ratio %.3f  spread %.3f" %
                      (C, cp, tiles, 1e3 * np.median(ra), leg["ms_per_pass"], 1e3 * np.median(rb), leg["atx2_ms_per_pass"], leg["ratio"],
                       leg["spread"]), flush=True)
            for v in xs + za + zb:
                v.free()
            sh.close()
    os.environ.pop("GV_ATXM_COLS", None)
    os.environ.pop("GV_ATXM_TILES", None)
    os.environ.pop("GV_ATXM_KERNEL", None)

    # for context: the same batches through a route-0 context (fp64 VALU kernels, ceil(C / 2) passes)
    route0 = []
    sh = shard(0)
    xs, za = [sh.vecN(y) for y in Y], [sh.vecM() for _ in range(cmax)]
    for C in counts:
        fn = lambda C=C: sh.atxm_dev(xs[:C], za[:C])
        fn()
        assert sh.atxm_info()["path"] == "fallback"
        reps = max(1, int(a.window / max(timed(sh, fn, 1), 1e-6)) + 1)
        ts = [timed(sh, fn, reps) for _ in range(a.rounds)]
        route0.append(dict(C=C, passes=sh.atxm_info()["passes"], ms=[1e3 * t for t in ts]))
        print("route 0  C=%2d  %8.3f ms" % (C, 1e3 * np.median(ts)), flush=True)
    for v in xs + za:
        v.free()
    sh.close()

    # the screens on route 1 under the library's own pick: product against panel and finishing kernels
    screens = []
    if a.screens:
        sh = shard(1)
        sh.set_screen_dosage(1)
        K = 10
        cov = [sh.vecN(np.concatenate([rng.standard_normal(a.N), np.zeros(npad - a.N)])) for _ in range(K)]
        sh.screen_cov_set(cov)
        for C in [int(t) for t in a.screens.split(",")]:
            ys = []
            for _ in range(C):
                y = np.zeros(npad)
                y[:a.N] = rng.standard_normal(a.N)
                ys.append(y)
            U = sh.screen_prepare(np.stack([y[:a.N] for y in ys]))
            us, yv = [sh.vecN(u) for u in U], [sh.vecN(y) for y in ys]
            outs = [[sh.vecM() for _ in range(C)] for _ in range(5)]
            prod = lambda: sh.atxm_dev(us, outs[0])
            marg = lambda: sh.screen_dev(us, outs[0], outs[1], outs[2])
            adj = lambda: sh.screen_cov_dev(yv, *outs)
            for fn in (prod, marg, adj):
                fn()
            info = sh.atxm_info()
            reps = max(1, int(a.window / max(timed(sh, marg, 1), 1e-6)) + 1)
            tp = [timed(sh, prod, reps) for _ in range(a.rounds)]
            tm = [timed(sh, marg, reps) for _ in range(a.rounds)]
            ta, parts = [], []
            for _ in range(a.rounds):
                ta.append(timed(sh, adj, 1))
                ci = sh.screen_cov_info()
                parts.append((ci["call_seconds_products"], ci["call_seconds_panel"]))
            screens.append(dict(C=C, K=K, path=info["path"], cols_per_pass=info["cols_per_pass"], product_ms=[1e3 * t for t in tp],
                                screen_ms=[1e3 * t for t in tm], screen_cov_ms=[1e3 * t for t in ta],
                                screen_cov_products_ms=[1e3 * p[0] for p in parts], screen_cov_panel_ms=[1e3 * p[1] for p in parts],
                                set_ms=1e3 * sh.screen_cov_info()["set_seconds"]))
            print("screens C=%2d  product %8.3f ms  gv_screen_dev %8.3f ms  gv_screen_cov_dev %8.3f ms (products %8.3f, panel %8.3f)" %
                  (C, 1e3 * np.median(tp), 1e3 * np.median(tm), 1e3 * np.median(ta), 1e3 * np.median([p[0] for p in parts]),
                   1e3 * np.median([p[1] for p in parts])), flush=True)
            for v in us + yv + [v for vs in outs for v in vs]:
                v.free()
        sh.close()

    res = dict(what="gv_atxm_dev on 8-bit dosage codes, route 1 (a) against ceil(C/2) gv_atx2_dev passes (b) on one context; ratio = b / a",
               N=a.N, M=a.M, rounds=a.rounds, window_s=a.window, seed=a.seed, legs=legs, route0=route0, screens=screens)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=os.path.relpath(out, ROOT), legs=len(legs))))


if __name__ == "__main__":
    main()
