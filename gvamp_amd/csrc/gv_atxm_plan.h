// gv_atxm_plan.h -- host-side planning of the multi-column product R = A^T Y (gv_atxm_dev, gv_atxm.hip).
// No HIP in here: tests/test_atxm_cpu.py compiles it with g++ into a stand-alone program.
//
// The passes, their uniform K-split and the choice of ks (`fill` = 24 work items per compute unit): gv_batch_plan.h.  Here a work item
// (segment s, quad q) = the four marker groups 4 q .. 4 q + 3 of 64 markers x the K-steps [b[s], b[s + 1]) of 256 individuals, items
// ordered segment-major (item = s * nq + q, dealt by block index) so that the workgroups resident together walk the same K range and
// share its digits through L2.
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
#include "gv_batch_plan.h"

namespace gvx {

using gvb::MAX_KS;
using gvb::I32_MAX;
using gvb::PREP_BLOCKS_MAX;
using gvb::up256;
using gvb::cp_for;
using gvb::equal_bounds;
using gvb::pass_of;
using gvb::pass_cols;

constexpr int64_t ENTRY_MAX = 384;                           // most a K-entry adds to a digit sum
constexpr int64_t SEG_INDIVIDUALS_MAX = I32_MAX / ENTRY_MAX; // 5 592 405
constexpr int CP_MAX = 8;

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

inline bool cp_ok(int cp) { return cp == 4 || cp == 8; }
// real individuals of segment [k0, k1) of K-steps
inline int64_t seg_individuals(int64_t k0, int64_t k1, int64_t N) {
    const int64_t lo = k0 * 256, hi = k1 * 256 < N ? k1 * 256 : N;
    return hi > lo ? hi - lo : 0;
}
inline bool bound_ok(int64_t N) { return N > 0 && N <= SEG_INDIVIDUALS_MAX; }

// N individuals, M > 0 markers, C > 0 columns, cp in {4, 8}; ks_pin > 0 pins the number of segments (clipped to the K-steps there
// are); fill: the work items a pass should have at least
inline Plan make_plan(int64_t N, int64_t M, int64_t C, int cp, int ks_pin, int64_t fill) {
    Plan p;
    if (N <= 0 || M <= 0 || C <= 0 || !cp_ok(cp) || ks_pin < 0 || ks_pin > MAX_KS) { p.err = 3; return p; }
    if (!bound_ok(N)) { p.err = 2; return p; }
    p.nrg = (M + 63) / 64;
    p.nkb = (N + 255) / 256;
    p.nq = (p.nrg + 3) / 4;
    p.ks = gvb::choose_ks(fill, p.nq, p.nkb, ks_pin);
    equal_bounds(p.nkb, p.ks, p.b);
    // a narrow batch takes a narrow instantiation
    p.cp = cp_for(C, cp);
    p.passes = (C + p.cp - 1) / p.cp;
    p.cp_last = cp_for(C - (p.passes - 1) * p.cp, p.cp);
    p.items = p.nq * p.ks;
    p.dig_bytes = up256((size_t)p.nkb * p.cp * 2048);
    p.part_bytes = up256((size_t)p.ks * p.cp * (size_t)(64 * p.nrg) * 64);
    p.small_bytes = gvb::scalar_bytes(p.cp);
    p.scratch_bytes = p.dig_bytes + p.part_bytes + p.small_bytes;
    return p;
}

}  // namespace gvx
