"""The numbering of the work items of the streaming kernels (gvm::item_cells in gv_mfma.h, the function the kernels call), checked on the
host: for a sweep of (quads, K-blocks, decomposition) the items cover every (quad, K-block) cell exactly once under both mappings, and
under the dealt mapping -- items drawn by ticket, big first -- the item sizes never increase with the item number (inside the balanced
remainder they are equal, but for the last range)."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "gv_mfma.h"
// argv: nq nkb ks skL piv taper geo xskew  ->  one line per mapping (0 block index, 1 dealt): "<mapping> <items> u:uend ..."
int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const long long nq = atoll(argv[1]), nkb = atoll(argv[2]);
    gvm::Decomp d;
    d.ks = atoi(argv[3]); d.skL = atoll(argv[4]); d.piv = atoll(argv[5]);
    d.taper = (float)atof(argv[6]); d.geo = (float)atof(argv[7]); d.xskew = (float)atof(argv[8]);
    const long long items = gvm::grid_of(d, nq, nkb);
    for (int deal = 0; deal < 2; deal++) {
        const gvm::KBounds kb = gvm::make_bounds(d, nkb, deal != 0);
        printf("%d %lld", deal, items);
        for (long long t = 0; t < items; t++) {
            const gvm::Item it = gvm::item_cells(d.skL > 0, deal != 0, (uint32_t)t, (uint32_t)items, (uint32_t)nq, (uint32_t)nkb,
                                                 (uint32_t)d.skL, (uint32_t)gvm::piv_of(d, nq), kb);
            printf(" %u:%u", it.u, it.uend);
        }
        printf("\n");
    }
    printf("grid %lld %lld %lld\n", (long long)gvm::deal_grid(items, 8), (long long)gvm::deal_grid(items, 16), (long long)gvm::deal_grid(items, 4));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("items")
    src = d / "items.cpp"
    src.write_text(SRC)
    out = d / "items"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "gvamp_amd", "csrc"),
                           "-I", "/opt/rocm/include", "-o", str(out), str(src)])
    return str(out)


def _cases():
    for nq, nkb in itertools.product((1, 2, 3, 7, 8, 37, 100), (1, 2, 9, 64, 257)):
        for ks in (1, 2, 3, 5, 24, 64):                               # uniform, tapered, geometric (xskew is ignored when dealt)
            if ks > nkb:
                continue
            yield (nq, nkb, ks, 0, 0, 0.0, 0.0, 0.0)
            if ks > 1:
                for taper, geo, xs in ((0.5, 0.0, 0.0), (0.9, 0.0, 0.02), (0.0, 0.5, 0.0), (0.0, 0.8, -0.035), (0.0, 0.0, 0.02)):
                    yield (nq, nkb, ks, 0, 0, taper, geo, xs)
        if nkb >= 2:
            for skl in sorted({8, 13, nkb, 3 * nkb + 1}):             # balanced
                yield (nq, nkb, 1, skl, 0, 0.0, 0.0, 0.0)
            for piv in sorted({1, nq // 2, nq - 1}):                  # hybrid: whole quads, then ranges no longer than a quad
                if 0 < piv < nq:
                    for skl in sorted({8, 13, nkb}):
                        if skl <= nkb:
                            yield (nq, nkb, 1, skl, piv, 0.0, 0.0, 0.0)


def test_items_cover_every_cell_once_and_never_grow(exe):
    ncase = 0
    for case in _cases():
        nq, nkb, ks, skl, piv = case[:5]
        lines = subprocess.check_output([exe] + [str(v) for v in case], text=True).splitlines()
        for ln in lines[:2]:
            f = ln.split()
            deal, items = int(f[0]), int(f[1])
            rng = [tuple(int(x) for x in t.split(":")) for t in f[2:]]
            assert len(rng) == items == (nq * ks if skl == 0 else piv + -(-(nq - piv) * nkb // skl)), case
            assert all(0 <= u < e <= nq * nkb for u, e in rng), (case, deal)
            covered = sorted(rng)                                     # a partition of [0, nq * nkb): each cell exactly once
            assert covered[0][0] == 0 and covered[-1][1] == nq * nkb, (case, deal)
            assert all(a[1] == b[0] for a, b in zip(covered, covered[1:])), (case, deal)
            if skl == 0:                                              # a segment stays inside its quad
                assert all(u // nkb == (e - 1) // nkb for u, e in rng), (case, deal)
            if deal:
                size = [e - u for u, e in rng]
                assert all(a >= b for a, b in zip(size, size[1:])), (case, size)
                if skl > 0:
                    assert all(s == nkb for s in size[:piv]) and all(s == skl for s in size[piv:-1]), (case, size)
        g8, g16, g4 = (int(x) for x in lines[2].split()[1:])
        for g, div in ((g8, 8), (g16, 16), (g4, 4)):                  # spare workgroups: at least 8, the same number for every XCD
            assert g % 8 == 0 and g - items >= max(8, items // div) and g - items < max(8, items // div) + 8, (case, g)
        ncase += 1
    assert ncase > 500
