// gv_atxm_plan.h -- host-side planning of the multi-column product R = A^T Y (gv_atxm_dev, gv_atxm.hip).
// No HIP in here: tests/test_atxm_cpu.py compiles it with g++ into a stand-alone program.
//
// A batch of C columns runs in ceil(C / CP) passes over the tile layout.  A pass is a uniform K-split: work item (segment s, quad q) =
// the four marker groups 4 q .. 4 q + 3 of 64 markers x the K-steps [b[s], b[s + 1]) of 256 individuals, b[j] = floor(nkb j / ks), items
// ordered segment-major (item = s * nq + q, dealt by block index) so that the workgroups resident together walk the same K range and
// share its digits through L2.  Every pass of a call uses the same split.
//
// ks is the smallest number of segments that gives a pass `fill` work items (24 per compute unit), but no segment is shorter than 8
// K-steps (the epilogue adds the segments up) and there are at most MAX_KS of them.  A pinned ks is clipped to the K-steps there are.
//
// The int32 bound: a K-entry adds at most 3 * 128 = 384 in magnitude to an int32 digit sum (plane value <= 3, balanced digit >= -128),
// no segment is longer than N individuals, and gv_set_dims admits N * 384 < 2^31 only.  The plan asserts it all the same (err 2).
//
// Scratch of a call, sized for its widest pass (cp columns) and reused by every pass -- the documented formula:
//   digits    nkb * cp * 2048                       8 bytes per individual of a K-step and column: 8 digit columns
//   partials  ks * cp * (64 * nrg) * 64             int32 digit planes X and Y: 2 x 8 digits per segment, column and marker
//   scalars   cp * (4 + 2 * PREP_BLOCKS_MAX) * 8    the four scalars of a column and the block partials of its preparation
// each rounded up to 256 bytes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gvx {

constexpr int MAX_KS = 64;                                   // = GV_MAX_KS
constexpr int64_t ENTRY_MAX = 384;                           // most a K-entry adds to a digit sum
constexpr int64_t I32_MAX = 2147483647LL;
constexpr int64_t SEG_INDIVIDUALS_MAX = I32_MAX / ENTRY_MAX; // 5 592 405
constexpr int PREP_BLOCKS_MAX = 1024;                        // doubles of block partials per column: 2 * PREP_BLOCKS_MAX (= gv_mfma.hip)
constexpr int CP_MAX = 8;
constexpr int MIN_SEG_STEPS = 8;

struct Plan {
    int err = 0;                 // 0 fine; 2 N * 384 does not fit an int32; 3 bad arguments
    int cp = 0;                  // columns per pass (4 or 8)
    int cp_last = 0;             // instantiation of the last pass: the narrowest of 4 / 8 that holds its columns
    int64_t passes = 0;
    int ks = 0;                  // K-segments
    int64_t nrg = 0, nkb = 0;    // marker groups of 64 markers, K-steps of 256 individuals
    int64_t nq = 0;              // quads of marker groups: ceil(nrg / 4)
    int64_t items = 0;           // nq * ks workgroups per pass
    uint32_t b[MAX_KS + 1] = {}; // segment s = K-steps [b[s], b[s + 1])
    size_t dig_bytes = 0, part_bytes = 0, small_bytes = 0, scratch_bytes = 0;
};

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
inline bool cp_ok(int cp) { return cp == 4 || cp == 8; }
// the narrowest instantiation that holds n columns, at most cp
inline int cp_for(int64_t n, int cp) {
    for (int w = 4; w < cp; w *= 2)
        if (n <= w) return w;
    return cp;
}
// real individuals of segment [k0, k1) of K-steps
inline int64_t seg_individuals(int64_t k0, int64_t k1, int64_t N) {
    const int64_t lo = k0 * 256, hi = k1 * 256 < N ? k1 * 256 : N;
    return hi > lo ? hi - lo : 0;
}
inline void equal_bounds(int64_t nkb, int ks, uint32_t* b) {
    for (int j = 0; j <= ks; j++) b[j] = (uint32_t)(nkb * j / ks);
}
inline bool bound_ok(int64_t N) { return N > 0 && N <= SEG_INDIVIDUALS_MAX; }
// column j of the batch is column j % cp of pass j / cp
inline int64_t pass_of(int64_t j, int cp) { return j / cp; }
inline int64_t pass_cols(int64_t p, int64_t C, int cp) { return C - p * cp < cp ? C - p * cp : cp; }

// N individuals, M > 0 markers, C > 0 columns, cp in {4, 8}; ks_pin > 0 pins the number of segments (clipped to the K-steps there
// are); fill: the work items a pass should have at least
inline Plan make_plan(int64_t N, int64_t M, int64_t C, int cp, int ks_pin, int64_t fill) {
    Plan p;
    if (N <= 0 || M <= 0 || C <= 0 || !cp_ok(cp) || ks_pin < 0 || ks_pin > MAX_KS) { p.err = 3; return p; }
    if (!bound_ok(N)) { p.err = 2; return p; }
    p.nrg = (M + 63) / 64;
    p.nkb = (N + 255) / 256;
    p.nq = (p.nrg + 3) / 4;
    if (ks_pin > 0) {
        p.ks = ks_pin > p.nkb ? (int)p.nkb : ks_pin;
    } else {
        int64_t ks = (fill + p.nq - 1) / p.nq, cap = p.nkb / MIN_SEG_STEPS;
        if (cap < 1) cap = 1;
        if (ks > cap) ks = cap;
        if (ks > MAX_KS) ks = MAX_KS;
        if (ks < 1) ks = 1;
        p.ks = (int)ks;
    }
    equal_bounds(p.nkb, p.ks, p.b);
    // a narrow batch takes a narrow instantiation
    p.cp = cp_for(C, cp);
    p.passes = (C + p.cp - 1) / p.cp;
    p.cp_last = cp_for(C - (p.passes - 1) * p.cp, p.cp);
    p.items = p.nq * p.ks;
    p.dig_bytes = up256((size_t)p.nkb * p.cp * 2048);
    p.part_bytes = up256((size_t)p.ks * p.cp * (size_t)(64 * p.nrg) * 64);
    p.small_bytes = up256((size_t)p.cp * (4 + 2 * PREP_BLOCKS_MAX) * 8);
    p.scratch_bytes = p.dig_bytes + p.part_bytes + p.small_bytes;
    return p;
}

}  // namespace gvx
