// gv_score_plan.h -- host-side planning of the multi-column product Z = A W (gv_score_dev, gv_score.hip).
// No HIP in here: tests/test_score_cpu.py compiles it with g++ into a stand-alone program.
//
// A batch of C columns runs in ceil(C / CP) passes over the tile layout.  A pass is a uniform K-split: work item (segment s, row
// group rg) = 256 individuals x the K-steps [b[s], b[s + 1]) of 64 markers, items ordered segment-major so that the workgroups
// resident together walk the same K range and share its digits through L2.  Every pass of a call uses the same split.
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
#include <cstddef>
#include <cstdint>

namespace gvs {

constexpr int MAX_KS = 64;                                   // = GV_MAX_KS
constexpr int64_t ENTRY_MAX = 512;                           // = gvm::GV_AX_ENTRY_MAX
constexpr int64_t I32_MAX = 2147483647LL;
constexpr int64_t SEG_MARKERS_MAX = I32_MAX / ENTRY_MAX;     // 4 194 303
constexpr int PREP_BLOCKS_MAX = 1024;                        // doubles of block partials per column: 2 * PREP_BLOCKS_MAX (= gv_mfma.hip)
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

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
inline bool cp_ok(int cp) { return cp == 4 || cp == 8 || cp == 16; }
// the narrowest instantiation that holds n columns, at most cp
inline int cp_for(int64_t n, int cp) {
    for (int w = 4; w < cp; w *= 2)
        if (n <= w) return w;
    return cp;
}
// real markers of segment [k0, k1) of K-steps
inline int64_t seg_markers(int64_t k0, int64_t k1, int64_t M) {
    const int64_t lo = k0 * 64, hi = k1 * 64 < M ? k1 * 64 : M;
    return hi > lo ? hi - lo : 0;
}
inline void equal_bounds(int64_t nkb, int ks, uint32_t* b) {
    for (int j = 0; j <= ks; j++) b[j] = (uint32_t)(nkb * j / ks);
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
// column j of the batch is column j % cp of pass j / cp
inline int64_t pass_of(int64_t j, int cp) { return j / cp; }
inline int64_t pass_cols(int64_t p, int64_t C, int cp) { return C - p * cp < cp ? C - p * cp : cp; }

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
        p.ks = ks_pin > p.nkb ? (int)p.nkb : ks_pin;
        if (!bound_ok(p.nkb, p.ks, M)) { p.err = 1; return p; }
    } else {
        // at least `fill` items, but no segment shorter than 8 K-steps (the epilogue adds the segments up)
        int64_t ks = (fill + p.nrg - 1) / p.nrg, cap = p.nkb / 8;
        if (cap < 1) cap = 1;
        if (ks > cap) ks = cap;
        if (ks > MAX_KS) ks = MAX_KS;
        if (ks < p.min_ks) ks = p.min_ks;
        while (ks <= MAX_KS && !bound_ok(p.nkb, (int)ks, M)) ks++;      // (rounding to whole K-steps)
        if (ks > MAX_KS) { p.err = 2; return p; }
        p.ks = (int)ks;
    }
    equal_bounds(p.nkb, p.ks, p.b);
    // a narrow batch takes a narrow instantiation
    p.cp = cp_for(C, cp);
    p.passes = (C + p.cp - 1) / p.cp;
    p.cp_last = cp_for(C - (p.passes - 1) * p.cp, p.cp);
    p.items = p.nrg * p.ks;
    p.dig_bytes = up256((size_t)p.nkb * p.cp * 1024);
    p.part_bytes = up256((size_t)p.ks * p.cp * (size_t)(256 * p.nrg) * 32);
    p.small_bytes = up256((size_t)p.cp * (4 + 2 * PREP_BLOCKS_MAX) * 8);
    p.scratch_bytes = p.dig_bytes + p.part_bytes + p.small_bytes;
    return p;
}

}  // namespace gvs
