"""Two epilogues of one kernel, k_ld_block: the LD-score pass (gv_ld_scores) against the preconditioner's Gram
build (gvp::gram, section 13; gv_precond_info.build_seconds) on gv_synth_bed_ld genotypes, in one process.  Seconds and useful integer
MAC/s of both -- 4 products x N x the (j, k) entries delivered (the in-band entries of the scores, the clipped window squares of the
Grams); ratio_to_gram is the scores' rate over the Gram build's, i.e. how much of a block each epilogue delivers.  Writes one JSON file.

    python scripts/bench_ld.py --N 400000 --M 125000 --out profiles/ld_bench_400k_125k.json

--kind dosage8: gv_ld_scores on 8-bit dosage codes (gv_set_ld_dosage), three contexts holding the same
gv_synth_dosage_na(seed, 8, 0) codes -- no reserved code among them -- timed alternately in one process: the one-product kernel with a
block edge of 128 and of 64 markers (GV_LD_DOSAGE_EDGE), and the four-product kernel forced by GV_DOSAGE_NA_KERNELS=1.  Per leg: seconds,
useful and computed integer MAC/s (computed: every 64 x 64 sub-block the launch multiplied, over the K-steps of 128 individuals) and the
implied load rate, 2 * EDGE * N bytes per block.

    python scripts/bench_ld.py --kind dosage8 --N 20000 --M 800000 --out profiles/ld_dosage_bench_20000x800000.json

--kind pos: gv_ld_scores_pos on synthetic base-pair positions, 1 kb between neighbours (so --wind-kb X reaches X
markers on each side and the index window of gv_ld_scores at B = X computes the same blocks: both are timed in the same process), or
with --pos-cluster alternating stretches of 2048 markers 0.25 kb and 4 kb apart (no index window equals that band).  --ncat C ...: a
random 0 / 1 annotation of C categories at the first --wind-kb (0 = no annotation).  One JSON line per call with seconds, block_pairs,
useful_macs, scratch_bytes and the pass count.

    python scripts/bench_ld.py --kind pos --wind-kb 512 2048 --ncat 1 16 64 97 --out profiles/ld_pos_400k_125k.json

--kind clump: gv_ld_clump on the same positions (1 kb between neighbours, the first --wind-kb) with a deterministic
synthetic p of which a share of 100 %, 5 % and 0.5 % of the markers is eligible (p <= p2 = 0.01; every eligible marker may be an index,
p1 = p2), in a random order and -- at 100 % -- in the order of the marker index, the deep chain of dependencies.  Per leg: the seconds
of the call, of its block pass and of its selection, the rounds, the blocks launched against the blocks in band; gv_ld_scores_pos with
one category on the same window is timed in the same process and round.

    python scripts/bench_ld.py --kind clump --wind-kb 512 --out profiles/ld_clump_400k_125k.json
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


DOSAGE_LEGS = (("uniform128", dict(GV_LD_DOSAGE_EDGE="128"), 128, 1), ("uniform64", dict(GV_LD_DOSAGE_EDGE="64"), 64, 1),
               ("forced4", dict(GV_DOSAGE_NA_KERNELS="1"), 64, 4))


def dosage8(a):
    shards = {}
    for name, env, _, _ in DOSAGE_LEGS:          # the switches are read by gv_create, per context
        os.environ.update(env)
        sh = capi.Shard(a.N, a.M)
        for k in env:
            del os.environ[k]
        sh.synth_dosage_na(77, 8, 0)
        sh.set_ld_dosage(1)
        assert sh.dosage_info()["na_kernels"] == (name == "forced4")
        shards[name] = sh
    rounds = []
    kpad = (a.N + 127) // 128 * 128
    for rd in range(a.rounds):
        row = {"round": rd, "ld": []}
        for B in a.windows:
            for name, _, edge, products in DOSAGE_LEGS:
                shards[name].ld_scores(B)
                st = shards[name].ld_info()
                blocks = st["block_pairs"] // (edge // 64) ** 2
                row["ld"].append(dict(leg=name, window=B, seconds=st["seconds"], products=products, useful_macs=st["useful_macs"],
                                      useful_macs_per_s=st["useful_macs"] / st["seconds"],
                                      computed_macs_per_s=products * 4096.0 * st["block_pairs"] * kpad / st["seconds"],
                                      blocks=blocks, load_bytes_per_s=blocks * 2.0 * edge * a.N / st["seconds"],
                                      scratch_bytes=st["scratch_bytes"]))
        rounds.append(row)
        print(json.dumps(row), flush=True)
    for sh in shards.values():
        sh.close()
    with open(a.out, "w") as f:
        json.dump(dict(kind="dosage8", N=a.N, M=a.M, rounds=rounds), f)
        f.write("\n")


def positional(a):
    import numpy as np
    j = np.arange(a.M)
    if a.pos_cluster:
        gaps = np.where((j // 2048) % 2 == 0, 250.0, 4000.0)
        gaps[0] = 0.0
        pos = np.cumsum(gaps)
    else:
        pos = 1000.0 * j
    rng = np.random.default_rng(5)
    annots = {C_: (rng.random((a.M, C_)) < 0.3).astype(np.float64) for C_ in a.ncat if C_ > 0}
    rows = []

    def leg(sh, rd, what, call, **kw):
        res = call()
        st = sh.ld_info()
        if rd < 0:                           # the warm-up round: every shape of the timed rounds, not recorded
            return res
        row = dict(round=rd, call=what, seconds=st["seconds"], block_pairs=st["block_pairs"], useful_macs=st["useful_macs"],
                   useful_macs_per_s=st["useful_macs"] / st["seconds"], seconds_per_block=st["seconds"] / max(st["block_pairs"], 1),
                   scratch_bytes=st["scratch_bytes"], passes=sh.ld_last_passes(), **kw)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return res

    with capi.Shard(a.N, a.M) as sh:
        sh.synth_bed(77, 5000, ld_block=a.ld_block, ld_ppm=900000)
        sh.compute_markers_statistics()
        for rd in range(-1, a.rounds):
            for X in a.wind_kb:
                # the two legs in an order that alternates with the round: what runs first is not always the same call
                legs = [("index", lambda: leg(sh, rd, "gv_ld_scores", lambda: sh.ld_scores(int(X)), window=int(X))),
                        ("pos", lambda: leg(sh, rd, "gv_ld_scores_pos", lambda: sh.ld_scores_pos(pos, 1000.0 * X), wind_kb=X, ncat=0))]
                if a.pos_cluster:
                    legs = legs[1:]
                k = (rd + 1) % len(legs)
                res = {name: run() for name, run in legs[k:] + legs[:k]}
                if rd >= 0 and "index" in res:          # the same band: the same bits, at the size that is timed
                    eq = all(np.array_equal(res["pos"][i], res["index"][i], equal_nan=True) for i in (0, 1))
                    rows.append(dict(round=rd, wind_kb=X, bits_equal_index_window=bool(eq)))
                    print(json.dumps(rows[-1]), flush=True)
            for C_, an in annots.items():
                leg(sh, rd, "gv_ld_scores_pos", lambda: sh.ld_scores_pos(pos, 1000.0 * a.wind_kb[0], annot=an), wind_kb=a.wind_kb[0], ncat=C_)
    with open(a.out, "w") as f:
        json.dump(dict(kind="pos", N=a.N, M=a.M, ld_block=a.ld_block, layout="default", pos_cluster=bool(a.pos_cluster), calls=rows), f)
        f.write("\n")


def clump_summary(rows):
    """the per-round seconds of the scores call and of the 100 % block pass, the speed-up of the smaller shares over the 100 % share
    (medians of the call's seconds) and the selection's share of the call on the order by marker index"""
    def med(v):
        return sorted(v)[len(v) // 2]

    def secs(leg, key="seconds"):
        return [r[key] for r in rows if r.get("leg", r["call"]) == leg]

    full = "share 1, random order"
    out = dict(scores_pos_seconds=secs("gv_ld_scores_pos"), clump_full_seconds=secs(full), clump_full_block_seconds=secs(full, "block_seconds"))
    for share in ("0.05", "0.005"):
        out["speedup_share_%s" % share] = med(secs(full)) / med(secs("share %s, random order" % share))
    deep = "share 1, p increasing with the marker index"
    out["selection_share_of_call_index_order"] = med(secs(deep, "select_seconds")) / med(secs(deep))
    out["rounds_index_order"] = max(r["rounds"] for r in rows if r.get("leg") == deep)
    return out


def clump(a):
    import numpy as np
    M, X = a.M, a.wind_kb[0]
    pos = 1000.0 * np.arange(M)
    rng = np.random.default_rng(5)
    u = rng.random(M)
    # share -> p: the markers of u below the share get p = 0.01 u / share in (0, 0.01], the others p = 0.5
    legs = [("share %g, random order" % sh_, sh_, np.where(u < sh_, 0.01 * u / sh_, 0.5)) for sh_ in (1.0, 0.05, 0.005)]
    legs.append(("share 1, p increasing with the marker index", 1.0, 0.01 * (np.arange(M) + 1.0) / M))
    rows = []
    with capi.Shard(a.N, M) as sh:
        sh.synth_bed(77, 5000, ld_block=a.ld_block, ld_ppm=900000)
        sh.compute_markers_statistics()
        for rd in range(-1, a.rounds):          # (round -1 warms every shape up and is not recorded)
            sh.ld_scores_pos(pos, 1000.0 * X)
            st = sh.ld_info()
            in_band = st["block_pairs"]
            if rd >= 0:
                rows.append(dict(round=rd, call="gv_ld_scores_pos", wind_kb=X, ncat=0, seconds=st["seconds"], block_pairs=in_band))
                print(json.dumps(rows[-1]), flush=True)
            for name, share, p in legs:
                idx, n_index = sh.ld_clump(pos, 1000.0 * X, p, 0.01, 0.01, a.clump_r2)
                st, last = sh.ld_info(), sh.ld_clump_last()
                if rd >= 0:
                    rows.append(dict(round=rd, call="gv_ld_clump", leg=name, share=share, wind_kb=X, r2=a.clump_r2, seconds=st["seconds"],
                                     block_seconds=last["block_seconds"], select_seconds=last["select_seconds"], rounds=last["rounds"],
                                     n_e1=last["n_e1"], n_e2=last["n_e2"], n_index=n_index, blocks_launched=st["block_pairs"],
                                     blocks_in_band=in_band, useful_macs=st["useful_macs"], scratch_bytes=st["scratch_bytes"]))
                    print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(kind="clump", N=a.N, M=M, ld_block=a.ld_block, layout="default", calls=rows, summary=clump_summary(rows)), f)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["bed", "dosage8", "pos", "clump"], default="bed")
    ap.add_argument("--wind-kb", type=float, nargs="+", default=[512.0])
    ap.add_argument("--pos-cluster", action="store_true")
    ap.add_argument("--clump-r2", type=float, default=0.5)
    ap.add_argument("--ncat", type=int, nargs="*", default=[])
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--ld-block", type=int, default=64)
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 512, 2048])
    ap.add_argument("--gram-window", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kind == "dosage8":
        return dosage8(a)
    if a.kind == "pos":
        return positional(a)
    if a.kind == "clump":
        return clump(a)
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
