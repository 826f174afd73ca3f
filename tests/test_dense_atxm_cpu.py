"""The batch ATx of 8-bit dosage codes without a GPU: the host-only plan gvamp_amd/csrc/gv_dense_atxm_plan.h
compiled with g++ into a small program with its own main and held to the rules written out here -- passes and the narrow last pass,
every byte count, and the segment cut (the one gv_dense_mfma.hip uses for its own products) at the caps None / 256 / 64: whole K-steps,
never more than the cap or the int32 bound of 131 071 entries, every step covered once.  The same program runs once more under the
address and undefined-behaviour sanitizers.  And the driver: --screen-dosage is an option it knows, and without it the refusal of
--run-mode screen on dosage data is the line it was."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
SEG_MAX, KSTEP, QUANT_BLOCKS = 131071, 128, 1024

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "gv_dense_atxm_plan.h"
// argv[1]: a file of cases "N M C cp cap cus", one output line each:
//   "err cp cp_last passes blocks rows_p kpad steps seg_steps segs pair_dig pair_small dig part small scratch | pass:cols ..."
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long N, M, C, cap;
    int cp, cus;
    while (fscanf(f, "%lld %lld %lld %d %lld %d", &N, &M, &C, &cp, &cap, &cus) == 6) {
        const gvdx::Plan p = gvdx::make_plan(N, M, C, cp, cap, cus);
        printf("%d %d %d %lld %lld %lld %lld %lld %lld %d %zu %zu %zu %zu %zu %zu |", p.err, p.cp, p.cp_last, (long long)p.passes,
               (long long)p.blocks, (long long)p.rows_p, (long long)p.kpad, (long long)p.cut.steps, (long long)p.cut.seg_steps, p.cut.segs,
               p.pair_dig_bytes, p.pair_small_bytes, p.dig_bytes, p.part_bytes, p.small_bytes, p.scratch_bytes);
        for (long long q = 0; q < p.passes && !p.err; q++) printf(" %lld:%lld", q, (long long)gvdx::pass_cols(q, C, p.cp));
        printf("\n");
    }
    fclose(f);
    return 0;
}
"""

CS = (1, 2, 3, 4, 5, 8, 9, 17, 33)
CAPS = (SEG_MAX, 256, 64)                  # None (the library's bound), 256, 64
PLAN_CASES = [(N, M, C, cp, cap, cus)
              for N, M in ((1, 1), (5, 3), (63, 17), (130, 70), (200, 513), (1003, 700), (4099, 3001), (20000, 800000), (400000, 1000),
                           (140000, 70))
              for C in CS for cp in (4, 8) for cap in CAPS for cus in (256,)] + [(20000, 800000, 16, 8, SEG_MAX, 0), (300000, 64, 5, 8, 10 ** 9, 8)]
BAD_ARGS = [(0, 5, 1, 4, 64, 256), (5, 0, 1, 4, 64, 256), (5, 5, 0, 4, 64, 256), (5, 5, 1, 16, 64, 256), (5, 5, 1, 2, 64, 256),
            (5, 5, 1, 4, 0, 256)]


def up256(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_atxm")
    src = d / "plan.cpp"
    src.write_text(SRC)
    inc = ["-I", os.path.join(ROOT, "gvamp_amd", "csrc")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + inc + ["-o", str(d / "plan"), str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + inc +
                          ["-o", str(d / "plan_san"), str(src)])
    with open(d / "cases.txt", "w") as f:
        for c in PLAN_CASES + BAD_ARGS:
            f.write("%d %d %d %d %d %d\n" % c)
    return d


def _run(exe, path):
    return subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)


def test_plan_against_its_rules(built):
    res = _run(built / "plan", built / "cases.txt")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(PLAN_CASES) + len(BAD_ARGS)
    seen_narrow_last = seen_capped = seen_one_step = seen_many = seen_filled = False
    for key, line in zip(PLAN_CASES, lines):
        N, M, C, cp, cap, cus = key
        head, groups = line.split("|")
        (err, pcp, cp_last, passes, blocks, rows_p, kpad, steps, seg_steps, segs, pair_dig, pair_small, dig, part, small,
         scratch) = [int(t) for t in head.split()]
        assert err == 0, key
        assert blocks == -(-M // 128) and rows_p == 128 * blocks and kpad == -(-N // 128) * 128 and steps == -(-N // KSTEP), key
        # passes: each column once, in order; a narrow batch or a narrow last pass takes the narrowest instantiation that holds it
        per = [int(t.split(":")[1]) for t in groups.split()]
        assert pcp in (4, 8) and pcp <= cp and (pcp == cp or C <= pcp), key
        assert passes == -(-C // pcp) == len(per) and sum(per) == C and all(1 <= t <= pcp for t in per), key
        assert cp_last == (4 if per[-1] <= 4 else 8) and per[-1] <= cp_last <= pcp, key
        seen_narrow_last |= cp_last < pcp
        # the cut: whole K-steps, every step in exactly one segment, none longer than the cap and the int32 bound -- unless one K-step
        # already is (a cap under 128 entries gives one step per segment: the kernel's granule)
        assert segs == -(-steps // seg_steps) and seg_steps >= 1 and (segs - 1) * seg_steps < steps <= segs * seg_steps, key
        bound = min(cap, SEG_MAX)
        assert seg_steps * KSTEP <= bound or seg_steps == 1, key
        assert seg_steps * KSTEP * 128 * 128 <= 2 ** 31 - 1, key
        # the rule behind it: about 16 waves per compute unit, no segment under 8 steps, then the cap
        units = cus if cus > 0 else 256
        want = max(1, min(-(-16 * units // blocks), steps // 8))
        assert seg_steps == max(1, min(-(-steps // want), max(1, bound // KSTEP))), key
        seen_capped |= -(-steps // want) > max(1, bound // KSTEP)
        seen_one_step |= seg_steps == 1 and steps > 1
        seen_many |= segs > 8
        seen_filled |= want > 1 and -(-steps // want) <= bound // KSTEP
        # the scratch is the documented formula
        assert pair_dig == kpad * 16 and pair_small == (6 * QUANT_BLOCKS + 2) * 8, key
        assert dig == up256((pcp // 2) * pair_dig) and part == up256(segs * rows_p * pcp * 8 * 4), key
        assert small == up256((pcp // 2) * pair_small) and scratch == dig + part + small, key
    assert seen_narrow_last and seen_capped and seen_one_step and seen_many and seen_filled
    for key, line in zip(BAD_ARGS, lines[len(PLAN_CASES):]):
        assert int(line.split()[0]) == 3, key


def test_the_cut_at_the_three_caps_of_the_gpu_test(built):
    """N = 1003: 8 K-steps; the library's bound leaves one segment, 256 entries two steps per segment, 64 entries one"""
    res = _run(built / "plan", built / "cases.txt")
    got = {}
    for key, line in zip(PLAN_CASES, res.stdout.splitlines()):
        if key[:4] == (1003, 700, 5, 8):
            h = [int(t) for t in line.split("|")[0].split()]
            got[key[4]] = (h[7], h[8], h[9])
    assert got == {SEG_MAX: (8, 8, 1), 256: (8, 2, 4), 64: (8, 1, 8)}


def test_plan_under_the_sanitizers(built):
    """stand-alone: the same cases, the same lines, nothing reported"""
    plain = _run(built / "plan", built / "cases.txt")
    san = _run(built / "plan_san", built / "cases.txt")
    assert san.returncode == 0, san.stderr[-3000:]
    assert san.stderr.strip() == "" and san.stdout == plain.stdout


def test_the_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    from gvamp_amd import capi
    for name in ("gv_set_screen_dosage", "gv_get_screen_dosage"):
        assert re.search(r"\bint %s\(" % name, txt) and name in capi.EXPORTS
    assert "#define GV_ABI_VERSION 4" in txt
    for meth in ("set_screen_dosage", "get_screen_dosage"):
        assert callable(getattr(capi.Shard, meth))
    assert "gv_dense_atxm.hip" in __import__("gvamp_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture(scope="module")
def driver():
    import __graft_entry__ as g
    g.build()
    return EXE


def _driver(exe, args, cwd):
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(cwd), timeout=60)
    head = "\nardyh command line options:\n"
    assert r.stdout.startswith(head), r.stdout
    return r.returncode, r.stdout[r.stdout.index("\n\n", len(head)) + 2:]


def test_the_driver_knows_the_option_and_keeps_its_refusal_without_it(driver, tmp_path):
    base = ["--run-mode", "screen", "--geno-format", "dosage8", "--bed-file", "x.bed", "--N", "8", "--Mt", "12"]
    status, text = _driver(driver, base, tmp_path)
    assert status == 1 and text == "FATAL: --run-mode screen works on 2-bit genotypes only, not on --geno-format dosage8\n"
    status, text = _driver(driver, base + ["--screen-dosage", "0"], tmp_path)
    assert status == 1 and text == "FATAL: --run-mode screen works on 2-bit genotypes only, not on --geno-format dosage8\n"
    # with the option the mode goes on to what it needs next: the phenotype files (no device work has happened)
    for fmt in ("dosage8", "dosage16"):
        status, text = _driver(driver, base[:3] + [fmt] + base[4:] + ["--screen-dosage", "1"], tmp_path)
        assert status == 1 and "works on 2-bit genotypes only" not in text
        assert text.endswith("FATAL  : no phen file(s) provided! Please use the --phen-files option.\n"), text
    r = subprocess.run([driver] + base + ["--screen-dosage", "2"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and "option --screen-dosage has to be 0 or 1" in r.stdout + r.stderr
