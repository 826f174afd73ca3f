"""LD clumping without a GPU (gv_ld_clump): the round scheme of the device selection against the sequential
definition (tests/clump_restatement.py) on random and on worst-case orders, a hand-computed case, and the host-side plan gvc::make_plan
(gvamp_amd/csrc/gv_ld_clump.h, no HIP in it) printed by a small g++ program and held to the restatement -- the ranks, E1 / E2, the
filtered list of blocks and the pair count.  The same program is built once more with the address and undefined-behaviour sanitizers
and run on its own."""
import math
import os
import subprocess

import numpy as np
import pytest

import clump_restatement as cr
import ld_pos_restatement as lpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gv_ld_clump.h"
#include "gv_ld_window.h"
// argv[1]: a file of cases "M radius has_chrom p1 p2  pos[0..M)  p[0..M)  chrom[0..M)" (hex floats, nan)  ->  per case one line
//   "<n_e1> <n_e2> <blocks_in_band> <pairs_e2> | rank[0..M) | order[0..n_e2) | I J I J ..."
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long M;
    int has_chrom;
    char tr[64], t1[64], t2[64], tok[64];
    while (fscanf(f, "%lld %63s %d %63s %63s", &M, tr, &has_chrom, t1, t2) == 5) {
        const double radius = strtod(tr, nullptr), p1 = strtod(t1, nullptr), p2 = strtod(t2, nullptr);
        std::vector<double> pos((size_t)M), p((size_t)M);
        std::vector<int> chrom((size_t)M);
        for (std::vector<double>* v : {&pos, &p})
            for (long long j = 0; j < M; j++) {
                if (fscanf(f, "%63s", tok) != 1) return 3;
                (*v)[(size_t)j] = strtod(tok, nullptr);
            }
        for (long long j = 0; j < M && has_chrom; j++)
            if (fscanf(f, "%d", &chrom[(size_t)j]) != 1) return 3;
        const gvw::Window w = gvw::make_window(pos.data(), has_chrom ? chrom.data() : nullptr, radius, M, 8192);
        if (w.verdict != gvw::OK) return 4;
        const gvc::Plan pl = gvc::make_plan(p.data(), p1, p2, w.hi.data(), w.dmax, M);
        printf("%lld %lld %lld %.0f |", (long long)pl.n_e1, (long long)pl.n_e2, (long long)pl.blocks_in_band, pl.pairs_e2);
        for (int r : pl.rank) printf(" %d", r);
        printf(" |");
        for (int j : pl.order) printf(" %d", j);
        printf(" |");
        for (int x : pl.pairs) printf(" %d", x);
        printf("\n");
    }
    fclose(f);
    return 0;
}
"""


def _random_r(M, seed, rho=0.8):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((50, M))
    for j in range(1, M):
        if j % 7:
            g[:, j] += rho * g[:, j - 1]
    r = np.corrcoef(g.T)
    poly = np.ones(M, dtype=bool)
    poly[[3, M // 2]] = False
    r[~poly] = 0.0
    r[:, ~poly] = 0.0
    return r, poly


def _chain(M):
    """neighbour-to-neighbour LD only: r_jk = 0.9 for |j - k| = 1, 0.1 otherwise"""
    j = np.arange(M)
    r = np.where(np.abs(j[:, None] - j[None, :]) == 1, 0.9, 0.1)
    r[np.diag_indices(M)] = 1.0
    return r, np.ones(M, dtype=bool)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rounds_equal_the_sequential_walk_on_random_orders(seed):
    M = 150
    r, poly = _random_r(M, seed)
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.exponential(1.0, M))
    chrom = np.repeat([4, 1], [100, 50])
    for p1, p2 in ((0.01, 0.02), (0.02, 0.02), (0.0, 0.02), (0.001, 0.5)):
        p = rng.random(M) * 0.03
        p[rng.integers(0, M, 5)] = math.nan
        p[7] = p[90] = p[91] = 0.004          # ties
        for r2 in (0.0, 0.2, 0.5, 1.0):
            adj = cr.adjacency(r, poly, pos, 6.0, chrom, p, p2, r2)
            assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
            want = cr.clump_sequential(adj, p, p1, p2)
            got = cr.clump_rounds(adj, p, p1, p2)
            assert _same(got, want), (p1, p2, r2)
            e1, e2 = cr.eligible(p, p1, p2)
            idx = want[0]
            assert (idx[~e2] == -1).all() and (idx[e1] >= 0).all()
            assert want[1] == int((idx == np.arange(M)).sum()) and (got[2] >= 1) == bool(e1.any())
            assert all(idx[i] == i for i in idx[idx >= 0])              # an index marker is its own index
            if p1 == 0.0:
                assert want[1] == 0 and got[2] == 0 and (idx == -1).all()


def test_rounds_equal_the_sequential_walk_on_worst_case_orders():
    M = 120
    r, poly = _chain(M)
    pos = np.arange(M) * 1.0
    for name, p, least in (("increasing: every marker waits for the one before", np.arange(M) * 1e-4, M - 1),
                           ("decreasing", np.arange(M)[::-1] * 1e-4, M - 1),
                           ("all equal: the index decides", np.zeros(M), M - 1),
                           ("alternating: two rounds", np.where(np.arange(M) % 2 == 0, 0.0, 1e-3), 2)):
        adj = cr.adjacency(r, poly, pos, 5.0, None, p, 1.0, 0.5)
        want = cr.clump_sequential(adj, p, 1.0, 1.0)
        got = cr.clump_rounds(adj, p, 1.0, 1.0)
        assert _same(got, want), name
        assert got[2] >= least, (name, got[2])
        assert got[2] <= M
    # the chain in increasing order: 0 an index, 1 claimed, 2 an index, ...
    p = np.arange(M) * 1e-4
    idx, n = cr.clump_sequential(cr.adjacency(r, poly, pos, 5.0, None, p, 1.0, 0.5), p, 1.0, 1.0)
    assert n == M // 2 and np.array_equal(idx, (np.arange(M) // 2) * 2)


def test_hand_computed_case():
    """eight markers on one chromosome, every pair in the band: a tie in p (0 and 1), a member-only marker that no index reaches (5), a
    NaN p (6) and a monomorphic index (7)"""
    M = 8
    pos = np.arange(M) * 1.0
    r = np.eye(M)
    for (j, k), v in {(0, 1): 0.9, (0, 2): -0.8, (1, 3): 0.75, (2, 3): 0.9, (3, 4): 0.6, (4, 5): 0.3, (0, 6): 0.95, (1, 4): -0.72}.items():
        r[j, k] = r[k, j] = v
    poly = np.ones(M, dtype=bool)
    poly[7] = False
    r[7, :] = r[:, 7] = 0.0
    p = np.array([1e-6, 1e-6, 1e-3, 1e-5, 5e-3, 8e-3, math.nan, 1e-7])
    p1, p2, r2 = 1e-4, 1e-2, 0.5
    e1, e2 = cr.eligible(p, p1, p2)
    assert list(np.nonzero(e1)[0]) == [0, 1, 3, 7] and list(np.nonzero(e2)[0]) == [0, 1, 2, 3, 4, 5, 7]
    assert list(cr.order_of(p, e1)) == [7, 0, 1, 3] and list(cr.order_of(p, e2)) == [7, 0, 1, 3, 2, 4, 5]
    adj = cr.adjacency(r, poly, pos, 100.0, None, p, p2, r2)
    edges = sorted((j, k) for j in range(M) for k in range(j + 1, M) if adj[j, k])
    assert edges == [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3)]          # (3, 4): 0.36 < 0.5; (0, 6): 6 is not in E2; (4, 5): 0.09
    # 7 first (monomorphic: a clump of one); 0 before 1 by the tie rule, claims 1 and 2; 3 is unassigned and becomes an index, but 1 and 2
    # are taken; 4 is adjacent to 1 only, which is no index; 5 is adjacent to nothing; 6 is not eligible
    want = np.array([0, 0, 0, 3, -1, -1, -1, 7])
    for f in (cr.clump_sequential, cr.clump_rounds):
        out = f(adj, p, p1, p2)
        assert np.array_equal(out[0], want) and out[1] == 3, f.__name__
    assert cr.clump_rounds(adj, p, p1, p2)[2] == 3          # 7 and 0 at once, then 1, then 3
    # the tie the other way round is no tie: with p_1 below p_0 marker 1 leads and takes 0, 3 and 4
    p[1] = 9e-7
    adj = cr.adjacency(r, poly, pos, 100.0, None, p, p2, r2)
    out = cr.clump_sequential(adj, p, p1, p2)
    assert np.array_equal(out[0], [1, 1, -1, 1, 1, -1, -1, 7]) and out[1] == 2
    assert _same(cr.clump_rounds(adj, p, p1, p2), out)
    # a radius that cuts (1, 3) and (1, 4)
    adj = cr.adjacency(r, poly, pos, 1.0, None, p, p2, r2)
    out = cr.clump_sequential(adj, p, p1, p2)
    assert np.array_equal(out[0], [1, 1, 3, 3, -1, -1, -1, 7]) and out[1] == 3
    assert cr.margin(r, lpr.in_band_pos(pos, 100.0), 0.5) == pytest.approx(0.72 * 0.72 - 0.5)          # the pair (1, 4)
    hi = lpr.window_hi(pos, 100.0)
    assert cr.blocks_launched(hi, e2) == 1 and cr.blocks_launched(hi, np.zeros(M, dtype=bool)) == 0


def _cases():
    """(name, pos, chrom or None, radius, p, p1, p2)"""
    rng = np.random.default_rng(12)
    M = 300
    j = np.arange(M)
    out = []
    p = rng.random(M) * 0.02
    out.append(("uniform, every marker a member", j * 1.0, None, 70.0, p, 0.01, 0.02))
    p = rng.random(M)
    p[[5, 77, 299]] = math.nan
    p[[10, 11, 200]] = 0.25
    out.append(("NaN and ties", np.cumsum(rng.exponential(1.0, M)), None, 30.0, p, 0.25, 0.5))
    p = np.ones(M)
    p[:64] = rng.random(64) * 0.01
    p[192:256] = rng.random(64) * 0.01
    out.append(("E2 in row groups 0 and 3 only", j * 1.0, None, 200.0, p, 0.005, 0.01))
    out.append(("... and a short reach", j * 1.0, None, 70.0, p, 0.005, 0.01))
    ch = np.repeat([2, 9, 4], [64, M - 65, 1])
    out.append(("three chromosomes", np.cumsum(rng.exponential(1.0, M)), ch, 90.0, rng.random(M) * 0.02, 0.001, 0.015))
    out.append(("nothing eligible", j * 1.0, None, 10.0, np.full(M, 0.5), 0.01, 0.02))
    out.append(("p1 = p2 = 1, all equal", j * 1.0, None, 10.0, np.zeros(M), 1.0, 1.0))
    out.append(("fewer than one row group", np.arange(40) * 1.0, None, 3.0, rng.random(40), 0.3, 0.6))
    out.append(("one marker", np.array([3.0]), None, 5.0, np.array([0.5]), 0.5, 0.5))
    big = 1000
    gaps = np.where((np.arange(big) // 100) % 2 == 0, 0.01, 7.0)
    p = np.where(rng.random(big) < 0.05, rng.random(big) * 0.01, 1.0)
    out.append(("clustered, 5 % eligible", np.cumsum(gaps), None, 1.0, p, 0.001, 0.01))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the program, plain and with the sanitizers, and the file of cases"""
    d = tmp_path_factory.mktemp("ldclump")
    src = d / "ldclump.cpp"
    src.write_text(SRC)
    inc = ["-I", os.path.join(ROOT, "gvamp_amd", "csrc")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + inc + ["-o", str(d / "ldclump"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc +
                          ["-o", str(d / "ldclump_san"), str(src)])
    with open(d / "cases.txt", "w") as f:
        for _, pos, ch, radius, p, p1, p2 in CASES:
            f.write("%d %s %d %s %s\n" % (pos.size, float(radius).hex(), ch is not None, float(p1).hex(), float(p2).hex()))
            f.write(" ".join(float(x).hex() for x in pos) + "\n")
            f.write(" ".join(float(x).hex() for x in p) + "\n")
            if ch is not None:
                f.write(" ".join(str(int(x)) for x in ch) + "\n")
    return d


def _run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)


def test_plan_header_against_the_restatement(built):
    res = _run(built / "ldclump", built / "cases.txt")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(CASES)
    for (name, pos, ch, radius, p, p1, p2), ln in zip(CASES, lines):
        head, ranks, order, pairs = ln.split("|")
        n1, n2, inband, npairs = (int(x) for x in head.split())
        M = pos.size
        e1, e2 = cr.eligible(p, p1, p2)
        want = cr.order_of(p, e2)
        assert (n1, n2) == (int(e1.sum()), int(e2.sum())), name
        got = np.array([int(x) for x in order.split()], dtype=np.int64)
        assert np.array_equal(got, want), name
        assert np.array_equal(got[:n1], cr.order_of(p, e1)), name          # E1 is the head of the order
        rank = np.array([int(x) for x in ranks.split()], dtype=np.int64)
        wr = np.full(M, -1, dtype=np.int64)
        wr[want] = np.arange(want.size)
        assert np.array_equal(rank, wr), name
        assert np.array_equal(rank >= 0, e2) and np.array_equal((rank >= 0) & (rank < n1), e1), name
        hi = lpr.window_hi(pos, radius, ch)
        pr_ = np.array([int(x) for x in pairs.split()], dtype=np.int64).reshape(-1, 2)
        assert inband == lpr.block_pairs(hi) and len(pr_) == cr.blocks_launched(hi, e2), name
        assert len({tuple(x) for x in pr_}) == len(pr_), name
        for I, J in pr_:
            assert I <= J and J <= int(hi[min(64 * I + 63, M - 1)]) // 64, name
            assert e2[64 * I:64 * I + 64].any() and e2[64 * J:64 * J + 64].any(), name
        assert npairs == cr.pairs_e2(pos, radius, ch, e2), name
    by = {c[0]: c for c in CASES}
    c = by["E2 in row groups 0 and 3 only"]
    hi = lpr.window_hi(c[1], c[3])
    assert cr.blocks_launched(hi, cr.eligible(c[4], c[5], c[6])[1]) == 3 < lpr.block_pairs(hi)          # (0, 0), (0, 3), (3, 3)
    c = by["... and a short reach"]
    assert cr.blocks_launched(lpr.window_hi(c[1], c[3]), cr.eligible(c[4], c[5], c[6])[1]) == 2
    c = by["nothing eligible"]
    assert cr.blocks_launched(lpr.window_hi(c[1], c[3]), cr.eligible(c[4], c[5], c[6])[1]) == 0


def test_plan_header_under_the_sanitizers(built):
    """stand-alone: the same cases, the same lines, nothing reported"""
    plain = _run(built / "ldclump", built / "cases.txt")
    san = _run(built / "ldclump_san", built / "cases.txt")
    assert san.returncode == 0, san.stderr[-3000:]
    assert san.stderr.strip() == "" and san.stdout == plain.stdout
