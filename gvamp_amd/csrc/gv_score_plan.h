// gv_score_plan.h -- host-side planning of the multi-column product Z = A W (gv_score_dev, gv_score.hip).
// No HIP in here: tests/test_score_cpu.py compiles it with g++ into a stand-alone program.
//
// The passes and their uniform K-split: gv_batch_plan.h.  Here a work item (segment s, row group rg) = 256 individuals x the K-steps
// [b[s], b[s + 1]) of 64 markers, items ordered segment-major so that the workgroups resident together walk the same K range and
// share its digits through L2.
//
// The int32 bound (gv_mfma.h, ax_bound_ok): a K-entry adds up to 512 in magnitude to an int32 digit sum, so no segment may span
// more than (2^31 - 1) / 512 = 4 194 303 real markers (the last K-step is clipped at M).
//
// Scratch of a call, sized for its widest pass (cp columns) and reused by every pass -- the documented formula:
//   digits    nkb * cp * 1024                       16 bytes per marker of a K-step and column: c and e, 8 digit columns each
//   partials  ks * cp * (256 * nrg) * 32            int32 digit planes: 8 digits per segment, column and row
//   scalars   cp * (4 + 2 * PREP_BLOCKS_MAX) * 8    the four scalars of a column and the block partials of its preparation
// each rounded up to 256 bytes.
#pragma once
#include "gv_batch_plan.h"

namespace gvs {

using gvb::MAX_KS;
using gvb::I32_MAX;
using gvb::PREP_BLOCKS_MAX;
using gvb::up256;
using gvb::cp_for;
using gvb::equal_bounds;
using gvb::pass_of;
using gvb::pass_cols;

constexpr int64_t ENTRY_MAX = 512;                           // = gvm::GV_AX_ENTRY_MAX
constexpr int64_t SEG_MARKERS_MAX = I32_MAX / ENTRY_MAX;     // 4 194 303
constexpr int CP_MAX = 16;

struct Plan {
    int err = 0;                 // 0 fine; 1 the pinned number of segments breaks the int32 bound; 2 no split of MAX_KS segments keeps it;
                                 // 3 bad arguments
    int cp = 0;                  // columns per pass (4, 8 or 16)
    int cp_last = 0;             // instantiation of the last pass: the narrowest of 4 / 8 / 16 that holds its columns
    int64_t passes = 0;
    int ks = 0;                  // K-segments
    int min_ks = 0;              // the fewest equal segments that keep the bound
    int64_t nrg = 0, nkb = 0;    // row groups of 256 individuals, K-steps of 64 markers
    int64_t items = 0;           // nrg * ks workgroups per pass
    uint32_t b[MAX_KS + 1] = {}; // segment s = K-steps [b[s], b[s + 1])
    size_t dig_bytes = 0, part_bytes = 0, small_bytes = 0, scratch_bytes = 0;
};

inline bool cp_ok(int cp) { return cp == 4 || cp == 8 || cp == 16; }
// real markers of segment [k0, k1) of K-steps
inline int64_t seg_markers(int64_t k0, int64_t k1, int64_t M) {
    const int64_t lo = k0 * 64, hi = k1 * 64 < M ? k1 * 64 : M;
    return hi > lo ? hi - lo : 0;
}
inline int64_t longest_segment(int64_t nkb, int ks, int64_t M) {
    int64_t longest = 0;
    for (int j = 0; j < ks; j++) {
        const int64_t m = seg_markers(nkb * j / ks, nkb * (j + 1) / ks, M);
        if (m > longest) longest = m;
    }
    return longest;
}
inline bool bound_ok(int64_t nkb, int ks, int64_t M) {
    return ks >= 1 && ks <= MAX_KS && ks <= nkb && longest_segment(nkb, ks, M) <= SEG_MARKERS_MAX;
}
// 0: a shard of more than MAX_KS * 4 194 303 markers cannot be served
inline int min_ks(int64_t nkb, int64_t M) {
    for (int64_t ks = (M + SEG_MARKERS_MAX - 1) / SEG_MARKERS_MAX; ks <= MAX_KS && ks <= nkb; ks++)
        if (ks >= 1 && bound_ok(nkb, (int)ks, M)) return (int)ks;
    return 0;
}

// N individuals, M > 0 markers, C > 0 columns, cp in {4, 8, 16}; ks_pin > 0 pins the number of segments (clipped to the K-steps there
// are); fill: the work items a pass should have at least -- eight per workgroup the
// device holds at once (three per compute unit), so that the last round of workgroups costs a few per cent, not half a pass
inline Plan make_plan(int64_t N, int64_t M, int64_t C, int cp, int ks_pin, int64_t fill) {
    Plan p;
    if (N <= 0 || M <= 0 || C <= 0 || !cp_ok(cp) || ks_pin < 0 || ks_pin > MAX_KS) { p.err = 3; return p; }
    p.nrg = (N + 255) / 256;
    p.nkb = (M + 63) / 64;
    p.min_ks = min_ks(p.nkb, M);
    if (!p.min_ks) { p.err = 2; return p; }
    if (ks_pin > 0) {
        p.ks = gvb::choose_ks(fill, p.nrg, p.nkb, ks_pin);         // the pin, clipped to the K-steps there are
        if (!bound_ok(p.nkb, p.ks, M)) { p.err = 1; return p; }
    } else {
        int ks = gvb::choose_ks(fill, p.nrg, p.nkb, 0, p.min_ks);
        while (ks <= MAX_KS && !bound_ok(p.nkb, ks, M)) ks++;      // (rounding to whole K-steps)
        if (ks > MAX_KS) { p.err = 2; return p; }
        p.ks = ks;
    }
    equal_bounds(p.nkb, p.ks, p.b);
    // a narrow batch takes a narrow instantiation
    p.cp = cp_for(C, cp);
    p.passes = (C + p.cp - 1) / p.cp;
    p.cp_last = cp_for(C - (p.passes - 1) * p.cp, p.cp);
    p.items = p.nrg * p.ks;
    p.dig_bytes = up256((size_t)p.nkb * p.cp * 1024);
    p.part_bytes = up256((size_t)p.ks * p.cp * (size_t)(256 * p.nrg) * 32);
    p.small_bytes = gvb::scalar_bytes(p.cp);
    p.scratch_bytes = p.dig_bytes + p.part_bytes + p.small_bytes;
    return p;
}

}  // namespace gvs
