// gv_dense_atxm_plan.h -- host-side planning of the multi-column product R = A^T Y on 8-bit dosage codes under the fixed-point route
// (gv_atxm_dev on gv_set_dosage_route(ctx, 1); gv_dense_atxm.hip).  No HIP in here:
// tests/test_dense_atxm_cpu.py compiles it with g++ into a stand-alone program.
//
// A batch of C columns runs in ceil(C / cp) passes over the resident pitched rows (gv_batch_plan.h: cp_for, pass_cols); every pass uses
// the K-segments of the one- and two-vector products.  cut_segments() below IS that cut -- gv_dense_mfma.hip calls it for its own
// shapes -- so the int32 invariant of gvdm::SEG_MAX has one place: no int32 accumulation spans more than `cap` <= seg_max K-entries,
// rounded DOWN to whole K-steps of the kernel, at least one.
//
// Scratch of a call, sized for its widest pass (cp columns) and reused by every pass:
//   digits    (cp / 2) * round128(N) * 16           a B-operand buffer per column pair: 16 digit columns per K-entry
//   partials  segs * (128 * blocks) * cp * 8 * 4    int32: whole 128-row blocks x segments x 8 digit columns per column
//   scalars   (cp / 2) * (6 * QUANT_BLOCKS + 2) * 8 per pair: 2 NB block maxima | 4 NB limb sums | 2 scalars
// each rounded up to 256 bytes.
#pragma once
#include "gv_batch_plan.h"

namespace gvdx {

using gvb::up256;
using gvb::cp_for;
using gvb::pass_cols;

constexpr int CP_MAX = 8;
constexpr int ATX_KSTEP = 128;             // individuals per step of the streaming kernel (= gvdm::ATX_KSTEP)
constexpr int64_t SEG_MAX = 131071;        // (= gvdm::SEG_MAX: (2^31 - 1) / (128 * 128))
constexpr int QUANT_BLOCKS = 1024;         // most blocks of a quantisation launch (= gvdm::BLOCKS)

struct Cut {
    int64_t steps = 1;              // K-steps in all
    int64_t seg_steps = 1;          // K-steps per segment
    int segs = 1;
};
// K entries in steps of kstep, `blocks` waves' worth of rows, at most cap (clipped to seg_max) entries per segment, cus compute units:
// about 16 waves per CU in all, a segment at least 8 steps long; the bound may only raise the number of segments
inline Cut cut_segments(int64_t K, int kstep, int64_t blocks, int64_t cap, int cus, int64_t seg_max = SEG_MAX) {
    Cut sh;
    sh.steps = (K + kstep - 1) / kstep;
    if (cap > seg_max) cap = seg_max;
    int64_t cap_steps = cap / kstep;
    if (cap_steps < 1) cap_steps = 1;
    int64_t want = ((int64_t)16 * (cus > 0 ? cus : 256) + blocks - 1) / (blocks > 0 ? blocks : 1);
    if (want > sh.steps / 8) want = sh.steps / 8;
    if (want < 1) want = 1;
    int64_t len = (sh.steps + want - 1) / want;
    if (len > cap_steps) len = cap_steps;
    if (len < 1) len = 1;
    sh.seg_steps = len;
    sh.segs = (int)((sh.steps + len - 1) / len);
    if (sh.segs < 1) sh.segs = 1;
    return sh;
}

struct Plan {
    int err = 0;                 // 0 fine; 3 bad arguments
    int cp = 0;                  // columns per pass (4 or 8)
    int cp_last = 0;             // instantiation of the last pass: the narrowest of 4 / 8 that holds its columns
    int64_t passes = 0;
    int64_t blocks = 0;          // blocks of 128 marker rows
    int64_t rows_p = 0;          // 128 * blocks: rows of a partial plane
    int64_t kpad = 0;            // N rounded up to 128: K-entries of a digit buffer
    Cut cut;
    size_t pair_dig_bytes = 0;   // one column pair's digit buffer
    size_t pair_small_bytes = 0; // one column pair's maxima, limb sums and scalars
    size_t dig_bytes = 0, part_bytes = 0, small_bytes = 0, scratch_bytes = 0;
};

inline bool cp_ok(int cp) { return cp == 4 || cp == 8; }

// N individuals, M > 0 markers, C > 0 columns, cp in {4, 8}, cap: most K-entries per int32 segment, cus: compute units
inline Plan make_plan(int64_t N, int64_t M, int64_t C, int cp, int64_t cap, int cus) {
    Plan p;
    if (N <= 0 || M <= 0 || C <= 0 || !cp_ok(cp) || cap < 1) { p.err = 3; return p; }
    p.blocks = (M + 127) / 128;
    p.rows_p = p.blocks * 128;
    p.kpad = (N + 127) / 128 * 128;
    p.cut = cut_segments(N, ATX_KSTEP, p.blocks, cap, cus);
    p.cp = cp_for(C, cp);
    p.passes = (C + p.cp - 1) / p.cp;
    p.cp_last = cp_for(C - (p.passes - 1) * p.cp, p.cp);
    p.pair_dig_bytes = (size_t)p.kpad * 16;
    p.pair_small_bytes = (size_t)(6 * QUANT_BLOCKS + 2) * 8;
    p.dig_bytes = up256((size_t)(p.cp / 2) * p.pair_dig_bytes);
    p.part_bytes = up256((size_t)p.cut.segs * (size_t)p.rows_p * (size_t)p.cp * 8 * 4);
    p.small_bytes = up256((size_t)(p.cp / 2) * p.pair_small_bytes);
    p.scratch_bytes = p.dig_bytes + p.part_bytes + p.small_bytes;
    return p;
}

}  // namespace gvdx
