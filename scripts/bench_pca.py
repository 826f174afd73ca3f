#!/usr/bin/env python3
"""One iteration of gv_pca_dev split into its two batch products and its panel kernels, and the panel step against the same
orthonormalise / Rayleigh-Ritz / rotate / residual sequence issued through gv_vec_dots and gv_vec_axpby.

One process, one synthetic shard, one context.  After a warm-up of both legs, in at least three alternating rounds:
  (a) gv_pca_dev for --iters iterations (tol below anything reachable, so every iteration runs): gv_pca_info gives the device time in
      the products and in the panel kernels (events on the context's stream; the call's one read-back per iteration synchronises),
      and a host clock around the call, which returns behind its last read-back, gives the wall time;
  (b) the panel step of ONE iteration -- CholeskyQR twice on Y, T = Q^T Y, U = Q V, R = Y V - U Theta, the norms of R -- with the Grams
      as gv_vec_dots batches of 8 pairs (the most a call takes), the small problems in numpy on the host and every panel update as gv_vec_axpby calls,
      a host clock around it ending in a device synchronise.
Every round goes to the JSON file; panel_ratio = median(b) / median(a's panel seconds per iteration), spread = the relative range of
the per-round ratios.  (b) is a host clock and holds its 68 read-backs, numpy's small problems and 766 calls through ctypes, (a)'s panel
seconds are device time: panel_ratio_host_clock puts (a) on the host clock too, as its wall time per iteration less the device time
of its products, which holds (a)'s read-back, host work and launch gaps.  The bytes of an iteration computed from the shapes are recorded beside the times.

    python scripts/bench_pca.py                        # N = 400 000 x M = 125 000, k = 10, L = 16: profiles/pca_400k_125k.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def primitives_panel_step(sh, Q, Y, U, R, k):
    """leg (b): one iteration's panel step on the panels Q, Y (lists of N-space vectors); Y ends orthonormal.  Returns the launches"""
    L = len(Q)
    launches = 0

    def gram(X, Z, pairs):
        nonlocal launches
        vals = []
        for i0 in range(0, len(pairs), 8):
            vals += list(sh.dots([(X[i], Z[j]) for i, j in pairs[i0:i0 + 8]]))
            launches += 1
        return vals

    full = [(i, j) for i in range(L) for j in range(L)]
    upper = [(i, j) for i in range(L) for j in range(i, L)]
    # Rayleigh-Ritz on (Q, Y)
    T = np.array(gram(Q, Y, full)).reshape(L, L)
    th, V = np.linalg.eigh(0.5 * (T + T.T))
    th, V = th[::-1], V[:, ::-1]
    for j in range(L):                                   # U = Q V
        sh.axpby(U[j], V[0, j], Q[0])
        for i in range(1, L):
            sh.axpby(U[j], V[i, j], Q[i], 1.0, U[j])
        launches += L
    for j in range(k):                                   # R = Y V - U Theta
        sh.axpby(R[j], -th[j], U[j])
        for i in range(L):
            sh.axpby(R[j], V[i, j], Y[i], 1.0, R[j])
        launches += L + 1
    r = np.sqrt(np.array(gram(R, R, [(j, j) for j in range(k)])))
    # Q <- orth(Y): CholeskyQR twice, in place (column j last to first, so that it reads the columns not yet replaced)
    for _ in range(2):
        S = np.zeros((L, L))
        for (i, j), v in zip(upper, gram(Y, Y, upper)):
            S[i, j] = S[j, i] = v
        Rinv = np.linalg.inv(np.linalg.cholesky(S).T)
        for j in range(L - 1, -1, -1):
            sh.axpby(Y[j], Rinv[j, j], Y[j])
            for i in range(j):
                sh.axpby(Y[j], Rinv[i, j], Y[i], 1.0, Y[j])
            launches += j + 1
    return launches, th, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400000)
    ap.add_argument("--M", type=int, default=125000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 3 and 1 <= a.k <= a.L <= 32
    from gvamp_amd import capi
    out = a.out or os.path.join(ROOT, "profiles", "pca_%dk_%dk.json" % (a.N // 1000, a.M // 1000))
    for v in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL", "GV_SCORE_COLS", "GV_SCORE_KS", "GV_SCORE_KERNEL"):
        os.environ.pop(v, None)
    rng = np.random.default_rng(a.seed)
    sh = capi.Shard(a.N, a.M)
    sh.set_layout(False, 2)
    sh.synth_bed(a.seed, 5000)
    sh.compute_markers_statistics()
    npad = 4 * sh.mbytes
    Q0 = np.zeros((a.L, npad))
    Q0[:, :a.N] = rng.standard_normal((a.L, a.N))
    q0, us = [sh.vecN(q) for q in Q0], [sh.vecN() for _ in range(a.k)]
    # leg (b)'s panels: Q orthonormal (numpy QR of the block), Y = G Q from the library's own products, restored before every round
    Qn = np.zeros((a.L, npad))
    Qn[:, :a.N] = np.linalg.qr(Q0[:, :a.N].T)[0].T
    Q = [sh.vecN(q) for q in Qn]
    B, Y0 = [sh.vecM() for _ in range(a.L)], [sh.vecN() for _ in range(a.L)]
    sh.atxm_dev(Q, B)
    sh.score_dev(B, Y0)
    for y in Y0:
        sh.axpby(y, a.N / a.M, y)
    Y, U, R = [sh.vecN() for _ in range(a.L)], [sh.vecN() for _ in range(a.L)], [sh.vecN() for _ in range(a.k)]

    def leg_a():
        sh.synchronize()
        t0 = time.perf_counter()
        ev, rs = sh.pca_dev(q0, us, 1e-300, a.iters)
        sh.synchronize()
        wall = time.perf_counter() - t0
        info = sh.pca_info()
        assert info["iterations"] == a.iters and info["converged"] == 0, info
        return dict(wall_s_per_iter=wall / a.iters, products_s_per_iter=info["seconds_products"] / a.iters,
                    panel_s_per_iter=info["seconds_panel"] / a.iters, theta=list(ev), resid=list(rs)), info

    def leg_b():
        for y, y0 in zip(Y, Y0):
            sh.copy(y, y0)
        sh.synchronize()
        t0 = time.perf_counter()
        launches, th, r = primitives_panel_step(sh, Q, Y, U, R, a.k)
        sh.synchronize()
        return dict(panel_s=time.perf_counter() - t0, launches=launches, theta=list(th[:a.k]), resid=list(r))

    info = leg_a()[1]
    leg_b()                                              # warm-up of both legs
    ra, rb = [], []
    for _ in range(a.rounds):
        ra.append(leg_a()[0])
        rb.append(leg_b())
    ratios = [b["panel_s"] / x["panel_s_per_iter"] for x, b in zip(ra, rb)]
    med = lambda key, rows: float(np.median([r[key] for r in rows]))                                   # noqa: E731
    wall, prod, pan = med("wall_s_per_iter", ra), med("products_s_per_iter", ra), med("panel_s_per_iter", ra)
    bytes_matrix = 2 * -(-a.L // 8) * (a.N * a.M // 4)              # the 2-bit matrix once per pass of 8 columns, two products
    # columns of npad doubles read or written per iteration: orth 2 x (Gram L + apply 2 L), T 2 L, U 2 L, R L + 2 k, its Gram k
    bytes_panel = (11 * a.L + 3 * a.k) * npad * 8
    res = dict(what="gv_pca_dev per iteration: the two batch products and the panel kernels (device events), and the panel step through "
                    "gv_vec_dots / gv_vec_axpby (b) over the panel kernels (a); panel_ratio = b / a",
               N=a.N, M=a.M, k=a.k, L=a.L, iters=a.iters, rounds=a.rounds, seed=a.seed, scratch_bytes=info["scratch_bytes"],
               atxm=sh.atxm_info(), score=sh.score_info(), pca_rounds=ra, primitives_rounds=rb,
               seconds_per_iteration=wall, products_s_per_iteration=prod, panel_s_per_iteration=pan,
               panel_share_of_iteration=pan / (prod + pan), host_and_gaps_s_per_iteration=wall - prod - pan,
               primitives_panel_s=med("panel_s", rb), primitives_launches=rb[0]["launches"],
               panel_ratio=med("panel_s", rb) / pan, panel_ratio_rounds=ratios,
               panel_host_clock_s_per_iteration=wall - prod, panel_ratio_host_clock=med("panel_s", rb) / (wall - prod),
               spread=float((max(ratios) - min(ratios)) / np.median(ratios)),
               bytes_matrix_per_iteration=bytes_matrix, bytes_panel_per_iteration=bytes_panel,
               panel_GBps=bytes_panel / pan / 1e9)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("seconds_per_iteration", "products_s_per_iteration", "panel_s_per_iteration",
                                          "panel_share_of_iteration", "primitives_panel_s", "primitives_launches", "panel_ratio", "panel_ratio_host_clock", "spread")}))


if __name__ == "__main__":
    main()
