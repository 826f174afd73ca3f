"""The scoring batch without a GPU (gv_score_dev): the host-only headers -- the column builder
gvamp_amd/csrc/host/score_cols.hpp and the plan gvamp_amd/csrc/gv_score_plan.h -- compiled into a small g++ program with its own main
and held to tests/score_restatement.py: the allele-unit conversion and its constant on markers that include monomorphic and all-missing
ones (msig = 1), the thresholding columns with ties exactly at a cut-off and index_of values -1, self and other, and for a grid of
(N, M, C, CP, ks) that every segment keeps the 4 194 303-marker bound, the grouping covers each column once and the scratch size is the
documented formula.  The same program is built once more with the address and undefined-behaviour sanitizers and run on its own."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import score_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gv_score_plan.h"
#include "host/score_cols.hpp"
static bool rd(FILE* f, std::vector<double>& v) {
    char tok[64];
    for (double& x : v) {
        if (fscanf(f, "%63s", tok) != 1) return false;
        x = strtod(tok, nullptr);
    }
    return true;
}
// argv[1]: a file of cases, one output line each
//   A M sqrtN  w[M] msig[M] mave[M]              ->  "A <K> | x[M]"                      (hex floats)
//   T M K  thr[K] w0[M] p[M] index_of[M]         ->  "T | col0[M] | col1[M] ..."
//   P N M C cp ks_pin fill                       ->  "P err cp cp_last passes ks min_ks nrg nkb items dig part small scratch | b[0..ks] |
//                                                      pass:cols ... | pass_of(j) ..."
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "A")) {
            long long M;
            char ts[64];
            if (fscanf(f, "%lld %63s", &M, ts) != 2) return 3;
            std::vector<double> w((size_t)M), msig((size_t)M), mave((size_t)M);
            if (!rd(f, w) || !rd(f, msig) || !rd(f, mave)) return 3;
            const std::vector<double> x = score_cols::allele_to_std(w.data(), msig.data(), (size_t)M, strtod(ts, nullptr));
            printf("A %a |", score_cols::allele_constant(w.data(), mave.data(), (size_t)M));
            for (double t : x) printf(" %a", t);
            printf("\n");
        } else if (!strcmp(kind, "T")) {
            long long M, K;
            if (fscanf(f, "%lld %lld", &M, &K) != 2) return 3;
            std::vector<double> thr((size_t)K), w0((size_t)M), p((size_t)M);
            std::vector<int64_t> idx((size_t)M);
            if (!rd(f, thr) || !rd(f, w0) || !rd(f, p)) return 3;
            for (int64_t& t : idx) {
                long long q;
                if (fscanf(f, "%lld", &q) != 1) return 3;
                t = q;
            }
            const auto cols = score_cols::threshold_columns(w0.data(), idx.data(), p.data(), (size_t)M, thr);
            printf("T");
            for (const auto& c : cols) {
                printf(" |");
                for (double t : c) printf(" %a", t);
            }
            printf("\n");
        } else if (!strcmp(kind, "P")) {
            long long N, M, C, fill;
            int cp, pin;
            if (fscanf(f, "%lld %lld %lld %d %d %lld", &N, &M, &C, &cp, &pin, &fill) != 6) return 3;
            const gvs::Plan p = gvs::make_plan(N, M, C, cp, pin, fill);
            printf("P %d %d %d %lld %d %d %lld %lld %lld %zu %zu %zu %zu |", p.err, p.cp, p.cp_last, (long long)p.passes, p.ks, p.min_ks,
                   (long long)p.nrg, (long long)p.nkb, (long long)p.items, p.dig_bytes, p.part_bytes, p.small_bytes, p.scratch_bytes);
            for (int j = 0; j <= p.ks && !p.err; j++) printf(" %u", p.b[j]);
            printf(" |");
            for (long long q = 0; q < p.passes && !p.err; q++) printf(" %lld:%lld", q, (long long)gvs::pass_cols(q, C, p.cp));
            printf(" |");
            for (long long j = 0; j < C && !p.err; j++) printf(" %lld", (long long)gvs::pass_of(j, p.cp));
            printf("\n");
        } else
            return 4;
    }
    fclose(f);
    return 0;
}
"""


def _allele_cases():
    rng = np.random.default_rng(3)
    out = []
    for M, N in ((1, 9), (57, 301), (700, 1003)):
        w = rng.standard_normal(M) * 10.0 ** rng.integers(-8, 8, M)
        msig = 1.0 / np.sqrt(rng.random(M) * 0.5 + 1e-3)
        mave = rng.random(M) * 2.0
        if M > 10:
            msig[[3, 9]] = 1.0                       # monomorphic (mave = 2) and all-missing (mave = 0): msig = 1
            mave[3], mave[9] = 2.0, 0.0
            w[5] = 0.0
            w[6] = -0.0
        out.append((w, msig, mave, math.sqrt(N)))
    return out


def _threshold_cases():
    rng = np.random.default_rng(4)
    M = 60
    w0 = rng.standard_normal(M)
    p = rng.random(M) * 0.1
    idx = np.where(rng.random(M) < 0.4, np.arange(M), rng.integers(0, M, M))       # self or another marker
    idx[rng.random(M) < 0.2] = -1
    idx[[0, 1, 2, 3]] = [0, 1, 2, 3]
    p[0], p[1], p[2], p[3] = 0.01, np.nextafter(0.01, 1.0), np.nextafter(0.01, 0.0), math.nan     # ties exactly at a cut-off
    idx[10], p[10] = 11, 0.0                         # a member of another marker's clump, however small its p
    return [(w0, idx, p, [0.0, 0.01, 0.05, 1.0]), (w0[:1], np.array([0]), np.array([0.5]), [0.5]),
            (w0[:1], np.array([-1]), np.array([0.0]), [0.5])]


PLAN_CASES = [(N, M, C, cp, ks, fill)
              for N, M in ((8, 64), (1003, 517), (2100, 1100), (400000, 125000), (400000, 1000000), (8, 4194304 + 64), (8, 4194303),
                           (300, 3 * 4194303 + 1), (8, 64 * 4194303 + 1))
              for C in (1, 2, 3, 5, 8, 16, 17, 33)
              for cp in (4, 8, 16)
              for ks, fill in ((0, 512), (0, 6144), (1, 512), (3, 512), (64, 512))]
ALLELE, THRESH = _allele_cases(), _threshold_cases()


def _hex(v):
    return " ".join(float(x).hex() for x in v)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("score")
    src = d / "score.cpp"
    src.write_text(SRC)
    inc = ["-I", os.path.join(ROOT, "gvamp_amd", "csrc")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + inc + ["-o", str(d / "score"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc +
                          ["-o", str(d / "score_san"), str(src)])
    with open(d / "cases.txt", "w") as f:
        for w, msig, mave, s in ALLELE:
            f.write("A %d %s\n%s\n%s\n%s\n" % (len(w), float(s).hex(), _hex(w), _hex(msig), _hex(mave)))
        for w0, idx, p, thr in THRESH:
            f.write("T %d %d\n%s\n%s\n%s\n%s\n" % (len(w0), len(thr), _hex(thr), _hex(w0), _hex(p), " ".join(str(int(t)) for t in idx)))
        for c in PLAN_CASES:
            f.write("P %d %d %d %d %d %d\n" % c)
    return d


def _run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)


def _floats(txt):
    return np.array([float.fromhex(t) for t in txt.split()])


def test_headers_against_the_restatement(built):
    res = _run(built / "score", built / "cases.txt")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(ALLELE) + len(THRESH) + len(PLAN_CASES)
    it = iter(lines)
    for w, msig, mave, s in ALLELE:
        head, xs = next(it).split("|")
        k = float.fromhex(head.split()[1])
        want = sr.allele_constant(w, mave)
        assert k == want and math.copysign(1.0, k) == math.copysign(1.0, want)
        x = _floats(xs)
        assert np.array_equal(x.view(np.uint64), sr.allele_to_std(w, msig, s).view(np.uint64))
        if len(w) > 10:
            assert x[3] == w[3] * s and x[9] == w[9] * s              # msig = 1: the conversion is the scaling alone
            assert x[5] == 0.0 and x[6] == 0.0 and math.copysign(1.0, x[6]) == -1.0
        # the constant is within gamma_M sum |mave w| of the exact sum
        exact = sum((sr.Fraction(float(a)) * sr.Fraction(float(b)) for a, b in zip(mave, w)), sr.Fraction(0))
        mag = sum((abs(sr.Fraction(float(a)) * sr.Fraction(float(b))) for a, b in zip(mave, w)), sr.Fraction(0))
        u = sr.Fraction(1, 2 ** 53)
        assert abs(sr.Fraction(k) - exact) <= len(w) * u / (1 - len(w) * u) * mag
    for w0, idx, p, thr in THRESH:
        parts = next(it).split("|")[1:]
        want = sr.threshold_columns(w0, idx, p, thr)
        assert len(parts) == len(thr)
        for got, wnt in zip(parts, want):
            assert np.array_equal(_floats(got).view(np.uint64), wnt.view(np.uint64))
    w0, idx, p, thr = THRESH[0]
    cols = sr.threshold_columns(w0, idx, p, thr)
    assert cols[1][0] == w0[0] and cols[1][2] == w0[2] and cols[1][1] == 0.0 and cols[0][0] == 0.0       # p == t is in, the next double is out
    assert all(c[3] == 0.0 and c[10] == 0.0 for c in cols)                                          # NaN p; another marker's member
    assert all(np.all((a == 0) | (a == b)) for a, b in zip(cols, cols[1:]))                          # the columns are nested
    for (N, M, C, cp, ks_pin, fill) in PLAN_CASES:
        head, b, groups, passof = next(it).split("|")
        h = [int(t) for t in head.split()[1:]]
        want = sr.plan(N, M, C, cp, ks_pin, fill)
        assert h[0] == want["err"], (N, M, C, cp, ks_pin, fill)
        if want["err"]:
            # a pinned split that breaks the bound, or a shard that no split of 64 segments serves
            assert (h[0] == 1 and ks_pin > 0) or (h[0] == 2 and M > 64 * sr.SEG_MARKERS_MAX)
            continue
        keys = ("cp", "cp_last", "passes", "ks", "min_ks", "nrg", "nkb", "items", "dig", "part", "small", "scratch")
        assert dict(zip(keys, h[1:])) == {k: want[k] for k in keys}, (N, M, C, cp, ks_pin, fill)
        bb = [int(t) for t in b.split()]
        ks, nkb = want["ks"], want["nkb"]
        assert bb == want["b"] and bb[0] == 0 and bb[-1] == nkb and all(x < y for x, y in zip(bb, bb[1:]))     # no empty segment
        assert max(sr.seg_markers(x, y, M) for x, y in zip(bb, bb[1:])) <= sr.SEG_MARKERS_MAX                # the int32 bound
        assert sum(sr.seg_markers(x, y, M) for x, y in zip(bb, bb[1:])) == M
        assert ks >= want["min_ks"] >= -(-M // sr.SEG_MARKERS_MAX) and (ks_pin == 0 or ks == min(ks_pin, nkb))
        # the grouping covers each column once; the scratch is the documented formula
        per = [int(t.split(":")[1]) for t in groups.split()]
        assert sum(per) == C and all(1 <= t <= want["cp"] for t in per) and len(per) == want["passes"] == -(-C // want["cp"])
        po = [int(t) for t in passof.split()]
        assert [po.count(q) for q in range(len(per))] == per and po == sorted(po)
        assert want["cp"] in (4, 8, 16) and want["cp"] <= cp and (want["cp"] == cp or C <= want["cp"])
        assert per[-1] <= want["cp_last"] <= want["cp"]
        assert want["dig"] == sr.up256(nkb * want["cp"] * 1024) and want["part"] == sr.up256(ks * want["cp"] * 256 * want["nrg"] * 32)
        assert h[-1] == want["dig"] + want["part"] + want["small"]
    assert any(sr.plan(8, 4194304 + 64, 3, 16, 1, 512)["err"] == 1 for _ in (0,))
    assert sr.plan(8, 4194304 + 64, 3, 16, 0, 512)["ks"] >= 2 and sr.plan(8, 4194303, 3, 16, 1, 512)["err"] == 0


def test_headers_under_the_sanitizers(built):
    """stand-alone: the same cases, the same lines, nothing reported"""
    plain = _run(built / "score", built / "cases.txt")
    san = _run(built / "score_san", built / "cases.txt")
    assert san.returncode == 0, san.stderr[-3000:]
    assert san.stderr.strip() == "" and san.stdout == plain.stdout


def test_the_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    from gvamp_amd import capi
    for name in ("gv_score_dev", "gv_score", "gv_score_info"):
        assert re.search(r"\bint %s\(" % name, txt) and name in capi.EXPORTS
    assert "#define GV_ABI_VERSION 4" in txt and "gv_score_stats" in txt
    for meth in ("score_dev", "score", "score_info"):
        assert callable(getattr(capi.Shard, meth))
    import ctypes
    assert ctypes.sizeof(capi.ScoreStats) == 48
    assert "gv_score.hip" in __import__("gvamp_amd.build", fromlist=["SOURCES"]).SOURCES
