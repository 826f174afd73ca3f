"""The positional LD window without a GPU (gv_ld_scores_pos): the numpy restatement of tests/ld_pos_restatement.py
against ld_restatement and a hand-computed case, and the host-side window construction gvw::make_window (gvamp_amd/csrc/gv_ld_window.h,
no HIP in it) printed by a small g++ program and held to the brute force -- hi, dmax, the entry count and the verdict of every
refusal at the right marker.  The same program is built once more with the address and undefined-behaviour sanitizers and run on its own."""
import math
import os
import subprocess

import numpy as np
import pytest

import ld_pos_restatement as lpr
import ld_restatement as ldr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gv_ld_window.h"
// argv[1]: a file of cases "M radius has_chrom max_reach  pos[0..M)  chrom[0..M)" (hex floats)  ->  per case one line
//   "<verdict> <at> <reach> <dmax> <entries> | hi[0..M)"     (hi only when the verdict is 0)
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long M, max_reach;
    int has_chrom;
    char tok[64];
    while (fscanf(f, "%lld %63s %d %lld", &M, tok, &has_chrom, &max_reach) == 4) {
        const double radius = strtod(tok, nullptr);
        std::vector<double> pos((size_t)M);
        std::vector<int> chrom((size_t)M);
        for (long long j = 0; j < M; j++) {
            if (fscanf(f, "%63s", tok) != 1) return 3;
            pos[(size_t)j] = strtod(tok, nullptr);
        }
        for (long long j = 0; j < M && has_chrom; j++)
            if (fscanf(f, "%d", &chrom[(size_t)j]) != 1) return 3;
        const gvw::Window w = gvw::make_window(pos.data(), has_chrom ? chrom.data() : nullptr, radius, M, max_reach);
        printf("%d %lld %lld %lld %.0f |", (int)w.verdict, (long long)w.at, (long long)w.reach, (long long)w.dmax, w.entries);
        for (long long h : w.hi) printf(" %lld", h);
        printf("\n");
    }
    fclose(f);
    return 0;
}
"""

OK, NOT_FINITE, DECREASES, REAPPEARS, TOO_LONG = range(5)          # gvw::Verdict


def _cases():
    """(name, pos, chrom or None, radius, expected verdict, expected marker, expected reach)"""
    rng = np.random.default_rng(11)
    out = []
    M = 300
    out.append(("uniform", np.arange(M) * 1.0, None, 10.5, OK, -1, 0))
    out.append(("uniform, S + j and an integer radius", 37.0 + np.arange(M), None, 64.0, OK, -1, 0))
    gaps = np.where((np.arange(M) // 50) % 2 == 0, 0.01, 7.0)       # alternating dense and sparse stretches
    out.append(("clustered", np.cumsum(gaps), None, 1.0, OK, -1, 0))
    out.append(("random gaps", np.cumsum(rng.exponential(1.0, M)), None, 3.0, OK, -1, 0))
    out.append(("all equal", np.full(200, 4.25), None, 0.0, OK, -1, 0))
    out.append(("radius 0, distinct", np.arange(M) * 0.5, None, 0.0, OK, -1, 0))
    out.append(("radius 0, ties", np.repeat(np.arange(60) * 0.5, 5), None, 0.0, OK, -1, 0))
    out.append(("one marker", np.array([3.0]), None, 5.0, OK, -1, 0))
    out.append(("one marker, one chromosome id", np.array([3.0]), np.array([7]), 5.0, OK, -1, 0))
    for edge in (100, 128):          # a break inside a row group and at a multiple of 64; the positions start again behind it
        ch = np.where(np.arange(M) < edge, 3, 1)
        pos = np.where(np.arange(M) < edge, np.arange(M), np.arange(M) - edge) * 1.0
        out.append(("break at %d" % edge, pos, ch, 40.0, OK, -1, 0))
    ch = np.repeat([5, 2, 9, 4], [64, 36, 199, 1])
    out.append(("breaks at 64, 100 and M - 1", np.arange(M) * 1.0, ch, 1000.0, OK, -1, 0))
    big = 8300
    pos = np.concatenate([np.zeros(8193), 10.0 + np.arange(big - 8193)])
    out.append(("a reach of exactly 8192", pos, None, 1.0, OK, -1, 0))
    pos = np.concatenate([[-5.0, -5.0], np.zeros(8194), 10.0 + np.arange(big - 8196)])
    out.append(("a reach of 8193", pos, None, 1.0, TOO_LONG, 2, 8193))
    pos = np.arange(M) * 1.0
    pos[77] = 75.5
    out.append(("decreasing", pos, None, 2.0, DECREASES, 77, 0))
    pos = np.arange(M) * 1.0
    pos[5] = math.nan
    out.append(("NaN", pos, None, 2.0, NOT_FINITE, 5, 0))
    pos = np.arange(M) * 1.0
    pos[299] = math.inf
    out.append(("infinite", pos, None, 2.0, NOT_FINITE, 299, 0))
    ch = np.repeat([1, 2, 1], [50, 50, 200])
    out.append(("a chromosome id reappears", np.arange(M) * 1.0, ch, 2.0, REAPPEARS, 100, 0))
    pos = np.arange(M) * 1.0
    pos[40] = 1.0
    pos[90] = math.nan
    out.append(("the first offender is named", pos, ch, 2.0, DECREASES, 40, 0))
    return out


CASES = _cases()


def _run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the program, plain and with the sanitizers, and the file of cases"""
    d = tmp_path_factory.mktemp("ldwindow")
    src = d / "ldwindow.cpp"
    src.write_text(SRC)
    inc = ["-I", os.path.join(ROOT, "gvamp_amd", "csrc")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + inc + ["-o", str(d / "ldwindow"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc +
                          ["-o", str(d / "ldwindow_san"), str(src)])
    with open(d / "cases.txt", "w") as f:
        for _, pos, ch, radius, *_ in CASES:
            f.write("%d %s %d %d\n" % (pos.size, float(radius).hex(), ch is not None, lpr.LD_WINDOW_MAX))
            f.write(" ".join(float(p).hex() for p in pos) + "\n")
            if ch is not None:
                f.write(" ".join(str(int(x)) for x in ch) + "\n")
    return d


def test_window_header_against_the_brute_force(built):
    res = _run(built / "ldwindow", built / "cases.txt")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(CASES)
    for (name, pos, ch, radius, verdict, at, reach), ln in zip(CASES, lines):
        head, his = ln.split("|")
        v, a, rch, dmax, ent = head.split()
        assert int(v) == verdict, name
        if verdict != OK:
            assert int(a) == at and his.strip() == "", name
            if verdict == TOO_LONG:
                assert int(rch) == reach, name
            continue
        hi = np.array([int(x) for x in his.split()], dtype=np.int64)
        want = lpr.window_hi(pos, radius, ch)
        assert np.array_equal(hi, want), name
        assert np.all(np.diff(hi) >= 0) and np.all(hi >= np.arange(hi.size)), name
        assert int(dmax) == lpr.dmax_of(want), name
        if pos.size <= 400:          # the interval [lo, hi] is the brute-force band, and the entry count is its size
            j = np.arange(pos.size)
            lo = np.searchsorted(hi, j)                     # the first marker whose band reaches j
            band = (j[None, :] >= lo[:, None]) & (j[None, :] <= hi[:, None])
            assert np.array_equal(band, lpr.in_band_pos(pos, radius, ch)), name
            assert int(ent) == lpr.entries(pos, radius, ch), name
        else:
            assert int(ent) == pos.size + 2 * int((want - np.arange(pos.size)).sum()), name
    by = {c[0]: c for c in CASES}
    assert lpr.window_hi(by["a reach of exactly 8192"][1], 1.0)[0] == 8192
    assert lpr.dmax_of(lpr.window_hi(by["clustered"][1], 1.0)) >= 1
    assert lpr.window_hi(by["break at 128"][1], 40.0, by["break at 128"][2])[127] == 127


def test_window_header_under_the_sanitizers(built):
    """stand-alone: the same cases, the same lines, nothing reported"""
    plain = _run(built / "ldwindow", built / "cases.txt")
    san = _run(built / "ldwindow_san", built / "cases.txt")
    assert san.returncode == 0, san.stderr[-3000:]
    assert san.stderr.strip() == "" and san.stdout == plain.stdout


def _random_r(M, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((50, M))
    for j in range(1, M):
        if j % 7:
            g[:, j] += 0.8 * g[:, j - 1]
    r = np.corrcoef(g.T)
    poly = np.ones(M, dtype=bool)
    poly[[3, M // 2]] = False
    r[~poly] = 0.0
    r[:, ~poly] = 0.0
    return r, poly


@pytest.mark.parametrize("B", [1, 5, 64, 200])
@pytest.mark.parametrize("adjusted", [False, True])
def test_index_positions_restate_the_index_window(B, adjusted):
    M = 150
    r, poly = _random_r(M, 2)
    for chrom in (None, np.repeat([1, 2, 3], [64, 36, 50])):
        want = ldr.scores(r, poly, B, chrom, adjusted, 50.0)
        for S in (0, 37):
            got = lpr.scores_pos(r, poly, S + np.arange(M) * 1.0, float(B), chrom, adjusted, 50.0)
            assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
        assert np.array_equal(lpr.in_band_pos(np.arange(M) * 1.0, float(B), chrom), ldr.in_band(M, B, chrom))


def test_a_ones_column_is_no_annotation():
    M = 150
    r, poly = _random_r(M, 3)
    pos = np.cumsum(np.random.default_rng(3).exponential(1.0, M))
    chrom = np.repeat([4, 1], [100, 50])
    for adjusted in (False, True):
        a = lpr.scores_pos(r, poly, pos, 2.5, chrom, adjusted, 50.0)
        b = lpr.scores_pos(r, poly, pos, 2.5, chrom, adjusted, 50.0, annot=np.ones((M, 1)))
        assert b[0].shape == (M, 1)
        assert np.array_equal(a[0], b[0][:, 0], equal_nan=True) and np.array_equal(a[1], b[1])


def test_hand_computed_case():
    """five markers, two categories, a tie in position (markers 1 and 2) and a chromosome break behind marker 2"""
    pos = np.array([1.0, 2.0, 2.0, 5.0, 5.5])
    chrom = np.array([1, 1, 1, 2, 2])
    r = np.eye(5)
    for (j, k), v in {(0, 1): 0.5, (0, 2): 0.2, (1, 2): 0.1, (3, 4): -0.4, (2, 3): 0.9, (0, 4): 0.7, (1, 3): -0.3}.items():
        r[j, k] = r[k, j] = v
    poly = np.ones(5, dtype=bool)
    annot = np.array([[1.0, 0.0], [2.0, -1.0], [0.0, 3.0], [1.0, 1.0], [-2.0, 0.5]])
    l2, n = lpr.scores_pos(r, poly, pos, 1.0, chrom, annot=annot)
    want = np.array([[1.0 + 0.25 * 2.0, 0.25 * -1.0 + 0.04 * 3.0],
                     [2.0 + 0.25 * 1.0, -1.0 + 0.01 * 3.0],
                     [0.04 * 1.0 + 0.01 * 2.0, 3.0 + 0.01 * -1.0],
                     [1.0 + 0.16 * -2.0, 1.0 + 0.16 * 0.5],
                     [-2.0 + 0.16 * 1.0, 0.5 + 0.16 * 1.0]])
    assert np.allclose(l2, want, rtol=0, atol=1e-15)
    assert np.allclose(want, [[1.5, -0.13], [2.25, -0.97], [0.06, 2.99], [0.68, 1.08], [-1.84, 0.66]], rtol=0, atol=1e-15)
    assert list(n) == [3, 3, 3, 2, 2]
    assert list(lpr.window_hi(pos, 1.0, chrom)) == [2, 2, 2, 4, 4]
    # half the radius: marker 0 is alone, the tie stays a pair, 5.5 - 5.0 <= 0.5 holds
    l2, n = lpr.scores_pos(r, poly, pos, 0.5, chrom, annot=annot)
    assert list(n) == [1, 2, 2, 2, 2] and list(lpr.window_hi(pos, 0.5, chrom)) == [0, 2, 2, 4, 4]
    assert np.array_equal(l2[0], annot[0]) and np.allclose(l2[1], [2.0, -1.0 + 0.01 * 3.0], rtol=0, atol=1e-15)
    # a monomorphic marker is no term of the others and has no score; the adjusted estimator with n = 12
    poly[1] = False
    r[1, :] = r[:, 1] = 0.0
    l2, n = lpr.scores_pos(r, poly, pos, 1.0, chrom, adjusted=True, nonas=12.0, annot=annot)
    f02 = 0.04 - 0.96 / 10.0
    assert np.isnan(l2[1]).all() and list(n) == [2, 0, 2, 2, 2]
    assert np.allclose(l2[0], [1.0 + f02 * 0.0, 0.0 + f02 * 3.0], rtol=0, atol=1e-15)
    # without chromosomes marker 2 does not reach marker 3 either (5 - 2 > 1), with radius 3 it does
    assert list(lpr.window_hi(pos, 1.0)) == [2, 2, 2, 4, 4] and list(lpr.window_hi(pos, 3.0)) == [2, 3, 3, 4, 4]
    assert list(lpr.window_hi(pos, 3.0, chrom)) == [2, 2, 2, 4, 4]
