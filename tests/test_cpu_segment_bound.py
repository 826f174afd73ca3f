"""The int32 bound of the Ax side (gvm::ax_bound_ok in gv_mfma.h, the predicate every admission path of gv_tune.hip asks) against the
segment boundaries gvm::make_bounds hands the kernels: a work item adds up to 512 per marker into an int32 digit sum, so the longest
K-segment of a decomposition, counted in real markers, times 512 must stay at or below 2^31 - 1.  The boundaries are printed by a
small host program and the longest segment is recomputed here, for both layouts (K-blocks of 256 / 64 markers), both mappings (dealt:
segments sorted longest first; block index: the xskew stretch), both quad parities."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1
ENTRY_MAX = 512                  # 3 * |digit(c)| + 1 * |digit(e)| of a missing genotype, digits down to -128
LIMIT = I32_MAX // ENTRY_MAX     # 4 194 303 markers

MS = [4194303, 4194304, 4194305, 5000000, 6000000, 6400000, 8000000, 8388606, 8388607, 8388608, 13000000, 20000000,
      64 * (2 ** 24 + 1)]
SMALL = [1, 300, 1000000]        # far below the bound: K-block counts below 64, 2 and 1
GEO = [(2, 0.5), (2, 0.35), (3, 0.5), (4, 0.5), (6, 0.6), (8, 0.65), (8, 0.8), (12, 0.7)]     # plan_decomps, build()
TAPERS = (0.0, 0.5, 0.9)
XSKEWS = (-0.2, 0.0, 0.2)
KB_MARKERS = {0: 256, 1: 64}     # layout 0: two stripe sets, 1: tile

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "gv_mfma.h"
// argv: M ...  ->  per M, layout, xskew and decomposition one line
//   "<M> <layout> <nkb> <min_ks> <xskew> <ks> <taper> <geo> <ok> <longest> | b.. | b.. | b.. | b.."   (mapping-major: block index parity 0, 1; dealt 0, 1)
static void one(long long M, int layout, float xskew, int ks, float taper, float geo) {
    const long long kbm = layout ? 64 : 256, nkb = (M + kbm - 1) / kbm;
    gvm::Decomp d;
    d.ks = ks; d.taper = taper; d.geo = geo; d.xskew = xskew;
    printf("%lld %d %lld %d %.2f %d %.2f %.2f %d %lld", M, layout, nkb, gvm::ax_min_ks(nkb, kbm, M), xskew, ks, taper, geo,
           gvm::ax_bound_ok(d, nkb, kbm, M) ? 1 : 0, (long long)gvm::ax_longest_item(d, nkb, kbm, M));
    if (ks >= 1 && ks <= 64 && ks <= nkb)
        for (int deal = 0; deal < 2; deal++) {
            const gvm::KBounds kb = gvm::make_bounds(d, nkb, deal != 0);
            for (int c = 0; c < 2; c++) {
                printf(" |");
                for (int j = 0; j <= ks; j++) printf(" %u", kb.b[c][j]);
            }
        }
    printf("\n");
}
int main(int argc, char** argv) {
    const float tapers[3] = {0.f, 0.5f, 0.9f}, xskews[3] = {-0.2f, 0.f, 0.2f};
    const int gks[8] = {2, 2, 3, 4, 6, 8, 8, 12};
    const float ggeo[8] = {0.5f, 0.35f, 0.5f, 0.5f, 0.6f, 0.65f, 0.8f, 0.7f};
    for (int a = 1; a < argc; a++) {
        const long long M = atoll(argv[a]);
        for (int layout = 0; layout < 2; layout++)
            for (float xs : xskews) {
                for (int ks = 1; ks <= 64; ks++)
                    for (float tp : tapers) one(M, layout, xs, ks, tp, 0.f);
                for (int g = 0; g < 8; g++) one(M, layout, xs, gks[g], 0.f, ggeo[g]);
            }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """every case of every M, from one run of the host program: {M: [case, ...]}"""
    d = tmp_path_factory.mktemp("segbound")
    src = d / "segbound.cpp"
    src.write_text(SRC)
    exe = d / "segbound"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "gvamp_amd", "csrc"),
                           "-I", "/opt/rocm/include", "-o", str(exe), str(src)])
    out = {}
    for ln in subprocess.check_output([str(exe)] + [str(m) for m in MS + SMALL], text=True).splitlines():
        head, *lists = ln.split(" |")
        f = head.split()
        case = dict(M=int(f[0]), layout=int(f[1]), nkb=int(f[2]), min_ks=int(f[3]), xskew=float(f[4]), ks=int(f[5]), taper=float(f[6]),
                    geo=float(f[7]), ok=f[8] == "1", longest=int(f[9]), bounds=[[int(x) for x in b.split()] for b in lists])
        out.setdefault(case["M"], []).append(case)
    return out


def longest_segment(case):
    """markers of the longest segment over both mappings and both quad parities, from the printed K-block boundaries"""
    M, kbm, nkb, ks = case["M"], KB_MARKERS[case["layout"]], case["nkb"], case["ks"]
    assert len(case["bounds"]) == 4
    longest = 0
    for b in case["bounds"]:
        assert len(b) == ks + 1 and b[0] == 0 and b[-1] == nkb and all(x < y for x, y in zip(b, b[1:])), case
        longest = max([longest] + [min(hi * kbm, M) - lo * kbm for lo, hi in zip(b, b[1:])])
    return longest


def ident(case):
    return {k: case[k] for k in ("M", "layout", "xskew", "ks", "taper", "geo")}


@pytest.mark.parametrize("M", MS + SMALL)
def test_predicate_agrees_with_the_boundaries_of_make_bounds(table, M):
    cases = table[M]
    assert len(cases) == 2 * 3 * (64 * 3 + len(GEO))
    assert {(c["ks"], c["geo"]) for c in cases if c["geo"] > 0} == set(GEO)
    assert {c["taper"] for c in cases} == set(TAPERS) and {c["xskew"] for c in cases} == set(XSKEWS)
    accepted = refused = 0
    for c in cases:
        assert c["nkb"] == -(-M // KB_MARKERS[c["layout"]])
        if c["ks"] > c["nkb"]:                       # no split into ks segments of at least one K-block exists
            assert not c["ok"] and c["longest"] == -1 and not c["bounds"], ident(c)
            continue
        longest = longest_segment(c)
        assert c["longest"] == longest, ident(c)
        assert c["ok"] == (longest * ENTRY_MAX <= I32_MAX), (ident(c), longest)
        accepted += c["ok"]
        refused += not c["ok"]
    if M <= LIMIT:
        assert refused == 0 and accepted > 0         # nothing with 1 <= ks <= min(64, nkb) is refused below the bound
    elif M <= 64 * LIMIT:
        assert accepted >= 1 and refused >= 1
    else:
        # 64 * (2^24 + 1) markers: 64 segments, the most a launch has (GV_MAX_KS), are at least 2^24 + 1 markers each, four times the
        # bound -- no decomposition can be accepted, and gv_set_dims refuses such a shard (ax_min_ks == 0)
        assert accepted == 0 and refused > 0 and all(c["min_ks"] == 0 for c in cases)


@pytest.mark.parametrize("M", MS + SMALL)
@pytest.mark.parametrize("layout", [0, 1])
def test_fewest_equal_segments(table, M, layout):
    """The uniform split of ks = ceil(M * 512 / (2^31 - 1)) equal segments is accepted -- but for the shards where the rounding to
    whole K-blocks makes its longest segment longer than M / ks (M = 8 388 606 / 8 388 607 on the stripe layout: two halves of 16 384
    K-blocks are 4 194 304 markers): there the fewest segments, which the tuner's fallback and its cost model start from
    (gvm::ax_min_ks), are the next ks, that one is accepted, and nothing with fewer segments is."""
    uni = {c["ks"]: c for c in table[M] if c["layout"] == layout and c["xskew"] == 0.0 and c["taper"] == 0.0 and c["geo"] == 0.0}
    min_ks = -(-M * ENTRY_MAX // I32_MAX)
    got = uni[1]["min_ks"]
    if min_ks > 64:
        assert got == 0 and not any(c["ok"] for c in uni.values())
        return
    if longest_segment(uni[min_ks]) * ENTRY_MAX <= I32_MAX:
        assert got == min_ks
    else:
        assert got == min_ks + 1 and -(-uni[min_ks]["nkb"] // min_ks) * KB_MARKERS[layout] > LIMIT >= M // min_ks
    assert uni[got]["ok"]
    assert not any(uni[ks]["ok"] for ks in range(1, got))
    # every variant of every split of fewer segments is refused too: ks >= ceil(M 512 / (2^31 - 1)) stays a necessary condition
    assert not any(c["ok"] for c in table[M] if c["layout"] == layout and c["ks"] < min_ks)


def test_the_splits_named_in_the_tuner_s_list_are_refused_where_their_first_segment_is_too_long(table):
    """ks 2 geo 0.5 / 0.35 and ks 2 taper 0.5 / 0.9 at M = 6 400 000: two segments are enough by count (min_ks = 2), and the first one of
    each is at least 4 194 305 markers -- refused on both layouts; the two equal halves are accepted."""
    for layout in (0, 1):
        sel = [c for c in table[6400000] if c["layout"] == layout and c["xskew"] == 0.0 and c["ks"] == 2]
        by = {(c["taper"], c["geo"]): c for c in sel}
        assert by[(0.0, 0.0)]["ok"] and by[(0.0, 0.0)]["min_ks"] == 2
        for key in ((0.0, 0.5), (0.0, 0.35), (0.5, 0.0), (0.9, 0.0)):
            assert not by[key]["ok"] and longest_segment(by[key]) >= 4194305, (layout, key, by[key]["longest"])
