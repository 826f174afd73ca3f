// gv_batch_plan.h -- what the plans of the batch products share (gv_score_plan.h: Z = A W, gv_atxm_plan.h: R = A^T Y).
// No HIP in here: the plan tests compile the two plan headers with g++ into stand-alone programs.
//
// A batch of C columns runs in ceil(C / CP) passes over the tile layout.  A pass is a uniform K-split into ks segments of K-steps,
// segment s = K-steps [b[s], b[s + 1]) with b[j] = floor(nkb j / ks), and every pass of a call uses the same split.  Each side keeps
// what is particular to it: its int32 bound, its geometry (row groups, K-steps, quads), its error codes and its digit / partial bytes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gvb {

constexpr int MAX_KS = 64;                 // most K-segments of a pass (= gvm::GV_MAX_KS)
constexpr int64_t I32_MAX = 2147483647LL;
constexpr int PREP_BLOCKS_MAX = 1024;      // a column's preparation leaves 2 * PREP_BLOCKS_MAX doubles of block partials (= RED_BLOCKS)
constexpr int MIN_SEG_STEPS = 8;           // no chosen segment is shorter than this many K-steps (the epilogue adds the segments up)

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
// the narrowest instantiation (4, 8, ...) that holds n columns, at most cp
inline int cp_for(int64_t n, int cp) {
    for (int w = 4; w < cp; w *= 2)
        if (n <= w) return w;
    return cp;
}
inline void equal_bounds(int64_t nkb, int ks, uint32_t* b) {
    for (int j = 0; j <= ks; j++) b[j] = (uint32_t)(nkb * j / ks);
}
// column j of the batch is column j % cp of pass j / cp
inline int64_t pass_of(int64_t j, int cp) { return j / cp; }
inline int64_t pass_cols(int64_t p, int64_t C, int cp) { return C - p * cp < cp ? C - p * cp : cp; }
// bytes of the four scalars of cp columns and of the block partials of their preparation
inline size_t scalar_bytes(int cp) { return up256((size_t)cp * (4 + 2 * PREP_BLOCKS_MAX) * 8); }
// K-segments of a pass over nkb K-steps whose segments are shared by `groups` work items each: a pin (> 0) is clipped to the K-steps
// there are; otherwise the fewest segments that give the pass `fill` work items, with no segment shorter than MIN_SEG_STEPS K-steps,
// at most MAX_KS of them, and at least floor_ks (the Ax side's int32 bound)
inline int choose_ks(int64_t fill, int64_t groups, int64_t nkb, int ks_pin, int floor_ks = 1) {
    if (ks_pin > 0) return ks_pin > nkb ? (int)nkb : ks_pin;
    int64_t ks = (fill + groups - 1) / groups, cap = nkb / MIN_SEG_STEPS;
    if (cap < 1) cap = 1;
    if (ks > cap) ks = cap;
    if (ks > MAX_KS) ks = MAX_KS;
    if (ks < floor_ks) ks = floor_ks;
    return (int)ks;
}

}  // namespace gvb
