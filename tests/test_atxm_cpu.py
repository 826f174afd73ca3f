"""The ATx batch without a GPU (gv_atxm_dev): the host-only plan gvamp_amd/csrc/gv_atxm_plan.h compiled into a
small g++ program with its own main and held to the rules written out here: for a grid of (N, M, C, cp, pin) the K-segments cover
[0, nkb) once and in order, none exceeds N individuals, N * 384 < 2^31 is asserted by the plan, ks follows its three rules (the fill,
no segment under 8 K-steps, at most 64), a pin is clipped to the K-steps there are, the last pass takes the narrowest instantiation
that holds it, and the scratch is the documented formula.  The same program is built once more with the address and
undefined-behaviour sanitizers and run on its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_KS, ENTRY_MAX, I32_MAX, PREP_BLOCKS_MAX = 64, 384, 2 ** 31 - 1, 1024

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "gv_atxm_plan.h"
// argv[1]: a file of cases "N M C cp ks_pin fill", one output line each:
//   "err cp cp_last passes ks nrg nkb nq items dig part small scratch | b[0..ks] | pass:cols ... | pass_of(j) ..."
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long N, M, C, fill;
    int cp, pin;
    while (fscanf(f, "%lld %lld %lld %d %d %lld", &N, &M, &C, &cp, &pin, &fill) == 6) {
        const gvx::Plan p = gvx::make_plan(N, M, C, cp, pin, fill);
        printf("%d %d %d %lld %d %lld %lld %lld %lld %zu %zu %zu %zu |", p.err, p.cp, p.cp_last, (long long)p.passes, p.ks, (long long)p.nrg,
               (long long)p.nkb, (long long)p.nq, (long long)p.items, p.dig_bytes, p.part_bytes, p.small_bytes, p.scratch_bytes);
        for (int j = 0; j <= p.ks && !p.err; j++) printf(" %u", p.b[j]);
        printf(" |");
        for (long long q = 0; q < p.passes && !p.err; q++) printf(" %lld:%lld", q, (long long)gvx::pass_cols(q, C, p.cp));
        printf(" |");
        for (long long j = 0; j < C && !p.err; j++) printf(" %lld", (long long)gvx::pass_of(j, p.cp));
        printf("\n");
    }
    fclose(f);
    return 0;
}
"""

N_LIMIT = I32_MAX // ENTRY_MAX            # 5 592 405: the most individuals gv_set_dims admits (N * 384 < 2^31)
PLAN_CASES = [(N, M, C, cp, ks, fill)
              for N, M in ((5, 3), (257, 65), (1003, 517), (2100, 1100), (400000, 125000), (50000, 1000000), (N_LIMIT, 64),
                           (N_LIMIT + 1, 64), (3000000, 200))
              for C in (1, 2, 3, 4, 5, 8, 9, 16, 17)
              for cp in (4, 8)
              for ks, fill in ((0, 512), (0, 6144), (1, 512), (3, 512), (64, 512))]
BAD_ARGS = [(0, 5, 1, 4, 0, 512), (5, 0, 1, 4, 0, 512), (5, 5, 0, 4, 0, 512), (5, 5, 1, 16, 0, 512), (5, 5, 1, 2, 0, 512),
            (5, 5, 1, 4, -1, 512), (5, 5, 1, 4, 65, 512)]


def up256(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("atxm")
    src = d / "atxm.cpp"
    src.write_text(SRC)
    inc = ["-I", os.path.join(ROOT, "gvamp_amd", "csrc")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + inc + ["-o", str(d / "atxm"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc +
                          ["-o", str(d / "atxm_san"), str(src)])
    with open(d / "cases.txt", "w") as f:
        for c in PLAN_CASES + BAD_ARGS:
            f.write("%d %d %d %d %d %d\n" % c)
    return d


def _run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)


def test_plan_against_its_rules(built):
    res = _run(built / "atxm", built / "cases.txt")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(PLAN_CASES) + len(BAD_ARGS)
    seen_narrow_last = seen_clip = seen_cap = seen_fill = False
    for (N, M, C, cp, pin, fill), line in zip(PLAN_CASES, lines):
        head, b, groups, passof = line.split("|")
        h = [int(t) for t in head.split()]
        key = (N, M, C, cp, pin, fill)
        if N * ENTRY_MAX >= 2 ** 31:                      # the int32 invariant is asserted by the plan itself
            assert h[0] == 2, key
            continue
        assert h[0] == 0, key
        err, pcp, cp_last, passes, ks, nrg, nkb, nq, items, dig, part, small, scratch = h
        assert nrg == -(-M // 64) and nkb == -(-N // 256) and nq == -(-nrg // 4), key
        # the ks rules: a pin is clipped to the K-steps there are; otherwise the smallest ks that reaches the fill, but no segment
        # shorter than 8 K-steps and at most 64 segments
        if pin:
            assert ks == min(pin, nkb), key
            seen_clip |= pin > nkb
        else:
            want = min(max(1, -(-fill // nq)), max(1, nkb // 8), MAX_KS)
            assert ks == want, key
            assert ks == 1 or nkb // ks >= 8, key
            assert ks * nq >= fill or ks == MAX_KS or ks == max(1, nkb // 8), key
            assert ks == 1 or (ks - 1) * nq < fill, key                                   # the smallest
            seen_cap |= ks == max(1, nkb // 8) and ks * nq < fill
            seen_fill |= ks * nq >= fill and ks > 1
        assert items == nq * ks, key
        # the segments: b[j] = floor(nkb j / ks), cover [0, nkb) once and in order, none empty, none longer than N individuals
        bb = [int(t) for t in b.split()]
        assert bb == [nkb * j // ks for j in range(ks + 1)], key
        assert bb[0] == 0 and bb[-1] == nkb and all(x < y for x, y in zip(bb, bb[1:])), key
        seg = [max(0, min(y * 256, N) - x * 256) for x, y in zip(bb, bb[1:])]
        assert sum(seg) == N and max(seg) <= N and max(seg) * ENTRY_MAX <= I32_MAX, key
        # passes: each column once, in order; a narrow batch or a narrow last pass takes the narrowest instantiation that holds it
        per = [int(t.split(":")[1]) for t in groups.split()]
        assert pcp in (4, 8) and pcp <= cp and (pcp == cp or C <= pcp), key
        assert passes == -(-C // pcp) == len(per) and sum(per) == C and all(1 <= t <= pcp for t in per), key
        po = [int(t) for t in passof.split()]
        assert [po.count(q) for q in range(len(per))] == per and po == sorted(po), key
        assert cp_last == (4 if per[-1] <= 4 else 8) and per[-1] <= cp_last <= pcp, key
        seen_narrow_last |= cp_last < pcp
        # the scratch is the documented formula
        assert dig == up256(nkb * pcp * 2048) and part == up256(ks * pcp * 64 * nrg * 64), key
        assert small == up256(pcp * (4 + 2 * PREP_BLOCKS_MAX) * 8) and scratch == dig + part + small, key
    assert seen_narrow_last and seen_clip and seen_cap and seen_fill
    for key, line in zip(BAD_ARGS, lines[len(PLAN_CASES):]):
        assert int(line.split()[0]) == 3, key


def test_plan_under_the_sanitizers(built):
    """stand-alone: the same cases, the same lines, nothing reported"""
    plain = _run(built / "atxm", built / "cases.txt")
    san = _run(built / "atxm_san", built / "cases.txt")
    assert san.returncode == 0, san.stderr[-3000:]
    assert san.stderr.strip() == "" and san.stdout == plain.stdout


def test_the_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    from gvamp_amd import capi
    for name in ("gv_atxm_dev", "gv_atxm", "gv_atxm_info", "gv_screen_dev"):
        assert re.search(r"\bint %s\(" % name, txt) and name in capi.EXPORTS
    assert "#define GV_ABI_VERSION 4" in txt and "gv_atxm_stats" in txt
    for meth in ("atxm_dev", "atxm", "atxm_info", "screen_dev", "screen"):
        assert callable(getattr(capi.Shard, meth))
    import ctypes
    assert ctypes.sizeof(capi.AtxmStats) == 48
    assert "gv_atxm.hip" in __import__("gvamp_amd.build", fromlist=["SOURCES"]).SOURCES
