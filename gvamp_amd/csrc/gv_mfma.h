// gv_mfma.h -- host-side plan and launchers of the fixed-point i8 MFMA family (gv_mfma.hip), and -- for HIP translation units, at
// the end -- the ONE copy of the device helpers of its fixed-point operand pipeline, shared with the batch products (gv_score.hip,
// gv_atxm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int RED_BLOCKS = 1024;   // most block partials of a reduction (gvk::dots, the prep launches)

namespace gvm {

struct Decomp {
    int ks = 1;          // uniform: K-segments per quad (workgroups per group of 4 row groups)
    int64_t skL = 0;     // > 0: balanced decomposition, cells (quad x K-block) per workgroup; 0: uniform K-split
    int64_t piv = 0;     // balanced only, > 0: hybrid -- the first piv quads go one per workgroup over the whole K range (in
                         // step, like a uniform split with ks = 1) and only the remaining quads are cut into ranges of skL cells
    int prio = 0;        // 1: waves lower their issue priority as they progress (k_mfma_matvec)
    float taper = 0.f;   // uniform split only: K-segment j is (1 + taper (ks-1-2j)/(ks-1)) times the mean length, so the
                         // workgroups dispatched last (the last segment) are the shortest and the launch's tail is short
    float geo = 0.f;     // uniform split only, 0 < geo < 1: K-segment j is geo^j times segment 0 (big first, geometrically
                         // smaller behind): the dispatcher hands the short workgroups out as slots free up, which evens out
                         // the 10-20 % spread in the time equal shares take (takes precedence over taper)
    int occ = 0;         // workgroups a CU may hold: 0 / 3 = what the registers allow (three), 2 = two (the launch reserves dynamic
                         // LDS to that end).  Fewer resident workgroups keep fewer K ranges and rows open at a time: the two-vector
                         // Ax of the 8-GPU shard on the tile layout streams 4 % faster with 512 than with 768 (profiles/r6_launch_dist_shard.txt),
                         // the 100 GB headline kernels 2-6 % slower -- one more thing the tuner measures
    float xskew = 0.f;   // uniform split, ks >= 2, block-index mapping only (GV_DEAL=0): workgroups are dealt to the eight XCDs round-robin by
                         // block index and four of the XCDs of an MI355X finish equal shares 4-6 % earlier than the other four (per-workgroup
                         // clocks: profiles/r6_shard_wgtime.txt), then idle for the rest of the launch.  On the boxes measured the early ones got
                         // the ODD block indices; WHICH hardware XCC ids those are changes with the box and the allocation (profiles/r6_xcd_skew.txt).
                         // The segments of a quad alternate between the two kinds; those with an odd block index are made 1 + xskew, the others
                         // 1 - xskew times their nominal length.  Headline Ax: 15.09 -> 14.90 ms at 0.025 on one box; the opposite sign loses as
                         // much.  Ignored when work items are dealt by ticket (Deal below): an XCD that is ahead then simply draws more items.
};
// dynamic LDS bytes that cap a CU at d.occ workgroups of the streaming kernels (160 KiB of LDS per CU; static LDS per workgroup: 8 KiB, or
// 4 KiB on the Ax side of the tile layout, 16 KiB in k_mfma_matvec MODE 3 / 6, plus 16 bytes for the ticket slot:
// 2 x (60000 + 16400) <= 163840 < 3 x (60000 + 4112).  A part with less LDS per CU could not launch occ = 2 at all.)
inline unsigned lds_pad_of(const Decomp& d) { return d.occ == 2 ? 60000u : 0u; }

// workgroups of a launch over nq quads x nkb K-blocks, and pieces (int32 partial sums per row) the epilogues add up at most
inline int64_t piv_of(const Decomp& d, int64_t nq) { return d.skL > 0 && d.piv > 0 ? (d.piv < nq ? d.piv : nq) : 0; }
inline int64_t grid_of(const Decomp& d, int64_t nq, int64_t nkb) {
    if (d.skL <= 0) return nq * d.ks;
    const int64_t piv = piv_of(d, nq);
    return piv + ((nq - piv) * nkb + d.skL - 1) / d.skL;
}
inline int64_t pieces_max(const Decomp& d, int64_t nkb) { return d.skL > 0 ? (nkb + d.skL - 1) / d.skL + 1 : d.ks; }

// ---- work items and how they are handed out ---------------------------------------------------------------------------
// A launch over nq quads x nkb K-blocks has grid_of() work ITEMS (one K-segment of one quad, one whole quad, or one balanced range
// of cells).  Which item a workgroup runs is decided in ONE place, item_cells(), shared by the kernels and the host (tests).
//   block-index mapping (ticket == NULL, GV_DEAL=0): item = blockIdx.x, the grid has exactly `items` workgroups, and the remainder
//       ranges of a hybrid decomposition come first;
//   dealt (Deal below): a workgroup draws t with one relaxed agent-scope atomic add and runs item t.  Items are numbered BIG FIRST
//       (uniform split: segment-major, segment lengths sorted longest first; balanced / hybrid: the whole quads, then the remainder
//       ranges), and the grid has SPARE workgroups: blocks go round-robin over the eight XCDs, so with grid == items an XCD that frees
//       its slots early could never run more than items / 8 of them.  With spare workgroups it starts them while tickets remain and takes
//       more than an eighth; a workgroup whose ticket is past the last item returns at once.  No workgroup ever waits for another, and
//       every item writes the partial-sum slots it always wrote: output is bit-identical by construction.
#if defined(__HIPCC__)
#define GV_HD __host__ __device__ __forceinline__
#else
#define GV_HD inline
#endif
// K-block boundaries of the segments of a uniform split (b[c][0] = 0 ... b[c][ks] = nkb; ks <= GV_MAX_KS).  [c]: the boundaries of a quad of
// parity c = q & 1 -- they differ only under Decomp::xskew with the block-index mapping
constexpr int GV_MAX_KS = 64;
struct KBounds { uint32_t b[2][GV_MAX_KS + 1]; };

struct Item {
    uint32_t u, uend;    // cells [u, uend) of the quad-major linearisation u = quad * nkb + K-block
    uint32_t r;          // uniform split: the segment number (= the piece the partial sums go to); balanced: index of the remainder range
};
// item t of `items` (t < items).  sk: balanced / hybrid (skL cells per range, the first piv quads whole); big_first: the dealt numbering
GV_HD Item item_cells(bool sk, bool big_first, uint32_t t, uint32_t items, uint32_t nq, uint32_t nkb, uint32_t skL, uint32_t piv,
                      const KBounds& kb) {
    Item it;
    if (sk) {
        const uint32_t U = nq * nkb, nrem = items - piv;      // ranges of the balanced remainder (piv == 0: all of them)
        const bool whole = big_first ? t < piv : t >= nrem;
        if (whole) {                                          // one whole quad
            it.r = 0;
            it.u = (big_first ? t : t - nrem) * nkb;
            it.uend = it.u + nkb;
        } else {
            it.r = big_first ? t - piv : t;
            it.u = piv * nkb + it.r * skL;
            it.uend = it.u + skL < U ? it.u + skL : U;
        }
    } else {
        // segment ks0 of quad q0, segment-major.  With an even number of quads the quads are rotated by one per segment row, so that under the
        // block-index mapping a quad's segments alternate between odd and even block indices either way (Decomp::xskew)
        const uint32_t ks0 = t / nq;
        uint32_t q0 = t % nq;
        if (!(nq & 1)) q0 = (q0 + ks0) % nq;
        it.r = ks0;
        it.u = q0 * nkb + kb.b[q0 & 1][ks0];
        it.uend = q0 * nkb + kb.b[q0 & 1][ks0 + 1];
    }
    return it;
}
// segment boundaries of a uniform split.  deal: the segments are sorted longest first and xskew is ignored
inline KBounds make_bounds(const Decomp& d, int64_t nkb, bool deal) {
    KBounds kb{};
    if (d.skL <= 0) {
        const int ks = d.ks < 1 ? 1 : (d.ks > GV_MAX_KS ? GV_MAX_KS : d.ks);
        // cumulative segment lengths, every segment at least one K-block (ks <= nkb): geometric (big first), tapered, or equal;
        // then, per quad parity c, the segments whose workgroup has an ODD block index ((c + j) odd) stretched by 1 + xskew, the others
        // shrunk by 1 - xskew
        const double xskew = deal ? 0.0 : (double)d.xskew;
        double w[GV_MAX_KS];
        for (int j = 0; j < ks; j++) {
            if (d.geo > 0.f && ks > 1) w[j] = j ? w[j - 1] * (double)d.geo : 1.0;
            else w[j] = ks > 1 ? 1.0 + (double)d.taper * (double)(ks - 1 - 2 * j) / (double)(ks - 1) : 1.0;
        }
        for (int c = 0; c < 2; c++) {
            double tot = 0.0, acc = 0.0, v[GV_MAX_KS];
            for (int j = 0; j < ks; j++) {
                v[j] = w[j] * (((c + j) & 1) ? 1.0 + xskew : 1.0 - xskew);      // (c + j) odd <-> odd block index
                tot += v[j];
            }
            kb.b[c][0] = 0;
            for (int j = 0; j < ks; j++) {
                acc += v[j];
                int64_t e = (int64_t)((double)nkb * acc / tot + 0.5);
                const int64_t lo = (int64_t)kb.b[c][j] + 1, hi = nkb - (ks - 1 - j);
                e = e < lo ? lo : (e > hi ? hi : e);
                kb.b[c][j + 1] = (uint32_t)e;
            }
            kb.b[c][ks] = (uint32_t)nkb;
            if (deal) {      // rounding leaves lengths that wobble by one K-block: longest first (insertion sort, ks <= 64)
                uint32_t len[GV_MAX_KS];
                for (int j = 0; j < ks; j++) len[j] = kb.b[c][j + 1] - kb.b[c][j];
                for (int j = 1; j < ks; j++) {
                    const uint32_t x = len[j];
                    int i = j - 1;
                    for (; i >= 0 && len[i] < x; i--) len[i + 1] = len[i];
                    len[i + 1] = x;
                }
                for (int j = 0; j < ks; j++) kb.b[c][j + 1] = kb.b[c][j] + len[j];
            }
        }
    }
    return kb;
}
// ---- the int32 bound of the Ax side -------------------------------------------------------------------------------------
// A work item adds up one int32 digit sum per row and column over ITS K-blocks, and the products are exact only while no such sum
// wraps.  On the ATx side K is the individuals: gv_set_dims refuses N * 384 >= 2^31 and no segment is longer than N.  On the Ax side
// K is the markers of the shard, which nothing limits, and one K-entry adds up to 512 in magnitude: MODE 1 / 4 store accX + accY as
// ONE plane, and a missing genotype contributes 3 * digit(c) + 1 * digit(e) with digits down to -128.  So the LONGEST item of an
// Ax-side decomposition, counted in real markers (kb_markers per K-block: 256 on the stripe layout, 64 on the tile layout; the last
// K-block is clipped at M), times 512 must not exceed 2^31 - 1.  Every path that admits an Ax-side decomposition asks ax_bound_ok():
// decomp_ok (gv_set_decomp, the cache file, the built-in table), the tuner's candidate list and its variants of a winner, the
// GV_KS_N override and the fallback (gv_tune.hip).  The segments of a uniform split are NOT equal -- geo, taper, xskew and the
// rounding to whole K-blocks -- so the number of segments alone decides nothing: the boundaries are those of make_bounds, for both
// quad parities and both mappings (a dealt context still launches by block index on a foreign stream).
constexpr int64_t GV_AX_ENTRY_MAX = 512;            // largest |contribution| of one K-entry to an int32 sum of the Ax side
constexpr int64_t GV_I32_MAX = 2147483647LL;
// markers of the longest item of decomposition d on the Ax side of a shard of M markers; -1: d is no decomposition of nkb K-blocks
inline int64_t ax_longest_item(const Decomp& d, int64_t nkb, int64_t kb_markers, int64_t M) {
    if (d.skL > 0) {     // balanced: at most skL cells, all of one quad's K range at most; hybrid: the whole quads span K
        const int64_t L = d.piv > 0 || d.skL > nkb ? nkb : d.skL;
        return L * kb_markers < M ? L * kb_markers : M;
    }
    if (d.ks < 1 || d.ks > GV_MAX_KS || d.ks > nkb) return -1;
    int64_t longest = 0;
    for (int deal = 0; deal < 2; deal++) {
        const KBounds kb = make_bounds(d, nkb, deal != 0);
        for (int c = 0; c < 2; c++)
            for (int j = 0; j < d.ks; j++) {
                const int64_t lo = (int64_t)kb.b[c][j] * kb_markers;
                int64_t hi = (int64_t)kb.b[c][j + 1] * kb_markers;
                if (hi > M) hi = M;
                if (hi - lo > longest) longest = hi - lo;
            }
    }
    return longest;
}
inline bool ax_bound_ok(const Decomp& d, int64_t nkb, int64_t kb_markers, int64_t M) {
    const int64_t longest = ax_longest_item(d, nkb, kb_markers, M);
    return longest >= 0 && longest * GV_AX_ENTRY_MAX <= GV_I32_MAX;
}
// the fewest equal K-segments that keep the bound: ceil(M * 512 / (2^31 - 1)), or one more where the rounding to whole K-blocks
// makes a segment longer than M / ks (M = 8 388 606 on the stripe layout: two halves of 16 384 K-blocks = 4 194 304 markers).
// 0: no split of at most GV_MAX_KS segments does (a shard of more than 64 * 4 194 303 markers)
inline int ax_min_ks(int64_t nkb, int64_t kb_markers, int64_t M) {
    if (M * GV_AX_ENTRY_MAX <= GV_I32_MAX) return 1;
    Decomp d;
    for (int64_t ks = (M * GV_AX_ENTRY_MAX + GV_I32_MAX - 1) / GV_I32_MAX; ks <= GV_MAX_KS && ks <= nkb; ks++) {
        d.ks = (int)ks;
        if (ax_bound_ok(d, nkb, kb_markers, M)) return d.ks;
    }
    return 0;
}
// The ticket counter of a context: one uint32 in device memory that is NEVER reset.  Launch k is handed base = the sum of the grid
// sizes of the launches before it and its workgroups compute t = old - base in unsigned arithmetic (both wrap together).  Every
// workgroup of every dealt launch draws exactly once -- before the `go` test of a device-resident CG step -- so the host's sum stays
// right when a pass is skipped on the device.  The launches that share a counter must run one after the other: they all go to `stream`
// (the context's stream); a launch on any other stream falls back to the block-index mapping.
struct Deal {
    uint32_t* ctr = nullptr;
    hipStream_t stream = nullptr;
    uint32_t base = 0;
    int spare_div = 8;       // spare workgroups = items / spare_div, at least 8 (GV_DEAL_SPARE, development)
};
// workgroups of a dealt launch: items + spare, rounded up so that every XCD gets the same number
inline int64_t deal_grid(int64_t items, int spare_div) {
    int64_t spare = spare_div > 0 ? items / spare_div : 0;
    if (spare < 8) spare = 8;
    return (items + spare + 7) / 8 * 8;
}

// ---- device-resident CG (gv_solvers.hip, cg_run_device) ------------------------------------------------------------
// State block of one CG system in device memory (doubles).  The kernels of a CG step read alpha / beta / the activity
// flags from it, so a step is enqueued without the host knowing the scalars of the previous one.
enum { ST_RZ = 0, ST_ALPHA, ST_BETA, ST_NORMV, ST_PREV_ONS, ST_ONS, ST_RELERR, ST_ACTIVE, ST_ITERS, ST_CONV, ST_NRELRES,
       ST_DENOISER, ST_STEPPED, ST_SIZE = 16 };
// What a pass over the shard needs to know when it is one half of a CG step.  Slot v = vector v of the pass.
struct CgHook {
    const int* go = nullptr;                 // the pass kernels return at once when *go == 0 (every system has finished)
    const double* state[2] = {nullptr, nullptr};   // slot v is CG system state[v]; NULL: not a CG system (a rider)
    // Ax side (k_prep_ax): the search direction is advanced on the way in, p <- z + beta p, when the system stepped
    double* p[2] = {nullptr, nullptr};
    const double* z[2] = {nullptr, nullptr};
    // ATx side (k_prep_atx): the same for an N-space system whose search direction is the operand of slot v (gv_cg_solve_aat2w)
    double* pn[2] = {nullptr, nullptr};
    const double* zn[2] = {nullptr, nullptr};
    // ATx side (k_fin_atx_dot): <out, addx> = <Q p, p>, block partials, then gvk::finalize -> dot_out[v][0]
    // Rider (gv_cg_extras.ride_x): while *ride == 1 and exactly one of the two systems has finished, the finished system's
    // slot of a two-vector Ax pass carries alt_x instead (decided on the device: the host learns of a finished system one
    // step late); the product lands in that slot's output, k_ride_copy moves it out and k_cgx_decide sets *ride = 2.
    const int* ride = nullptr;
    const double* alt_x = nullptr;
    double* ride_out = nullptr;              // != NULL: the Ax epilogue writes the rider's product there itself (no k_ride_copy)
    double* dot_part[2] = {nullptr, nullptr};
    double* dot_out[2] = {nullptr, nullptr};
    // Ax side (k_fin_ax), slot v closing an application of tau A A^T + gam2 I to dq_p[v] (gv_cg_solve_aat2w, one rank, vectors of at
    // most RED_BLOCKS * 256 entries): out = dq_tau * product + dq_gam2 * dq_p and the block partials of <out, dq_p> in dq_part[v],
    // while the system state[v] is running -- gvk::aat_step is then told that its k_aat_dq has been done (dq_done)
    const double* dq_p[2] = {nullptr, nullptr};
    double* dq_part[2] = {nullptr, nullptr};
    double dq_tau = 0.0, dq_gam2 = 0.0;
    bool dot_self = false;                   // the consumer adds the block partials of <out, addx> up itself: no gvk::finalize launch
};

struct Plan {
    int64_t M = 0, N = 0;
    int64_t nrg_m = 0, nkb_m = 0;   // stripes_m: row groups of 64 markers x K-blocks of 256 individuals
    int64_t nrg_n = 0, nkb_n = 0;   // stripes_n: row groups of 64 individuals x K-blocks of 256 markers
    // work decomposition of the streaming kernel, per kernel class: dm[0] ATx (MODE 0), dm[1] two-vector ATx / p-value sums
    // (MODE 2), dn[0] Ax and the people sums (MODE 1, 4), dn[1] two-vector Ax (MODE 3)
    Decomp dm[2], dn[2];
    void* stripes_m = nullptr;
    void* stripes_n = nullptr;
    // layout 1 ("tile", gv_set_layout(.., 2)): ONE resident re-encoding, 64 markers x 256 individuals per 4 KiB super-block,
    // serves both products (gv_mfma.hip).  Then nrg_m / nkb_m describe it (marker groups x individual blocks) and the Ax
    // side walks it transposed: nrg_n = nkb_m row groups of rows_n = 256 individuals, nkb_n = nrg_m K-steps of 64 markers.
    void* tiles = nullptr;
    int layout = 0;
    int rows_n = 64;                // rows per row group on the Ax side
    int64_t rstride_n = 0;          // tile layout, Ax side: row groups per K-step in memory when a launch covers a sub-range (0: nrg_n)
    void* dig0 = nullptr;           // digit buffers, max(nkb_m, nkb_n) * 2048 bytes each
    void* dig1 = nullptr;
    double* cv = nullptr;           // M doubles: c = msig * x
    double* ev = nullptr;           // M doubles: e = (mave - 3) * c
    double* cv2 = nullptr;          // the same for the second vector of a two-vector Ax
    double* ev2 = nullptr;
    double* scal = nullptr;         // 2 x 4 doubles: amax, sum, 2^(54-e), 2^(e-54) (second set: marker_sums2's p2)
    int32_t* partial = nullptr;     // per-(K-split, plane, row) digit sums
    size_t partial_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // when set: recorded around the matvec kernel launch (roofline timing)
    Deal* deal = nullptr;           // != NULL: work items are dealt by ticket (owned by the context; copies of a Plan share it)
};

void stripes_m_chunk(hipStream_t s, const uint8_t* raw, int64_t pitch, int64_t mc, int64_t N, void* stripes,
                     int64_t rg0, int64_t nkb);
void stripes_n_chunk(hipStream_t s, const uint8_t* raw, int64_t pitch, int64_t mc, int64_t N, void* stripes,
                     int64_t kb0, int64_t nkb, int64_t nrg_n);
void tile_chunk(hipStream_t s, const uint8_t* raw, int64_t pitch, int64_t mc, int64_t N, void* tiles, int64_t rg0, int64_t nkb);
void stats_from_tiles(hipStream_t s, const void* tiles, const uint32_t* mask2, int64_t M, int64_t nrg, int64_t nkb, int64_t P4,
                      double nonas, double alpha_scale, double* mave, double* msig, uint32_t* counts);
// counts (may be NULL): 3 per marker = present individuals with a = 2, 1, 0
void stats_from_stripes(hipStream_t s, const void* stripes_m, const uint32_t* mask2, int64_t M, int64_t nkb,
                        int64_t P4, double nonas, double alpha_scale, double* mave, double* msig, uint32_t* counts);
// The p-value pass (data::pvals_calc / pvals_calc_LOCO): p = mask (y - z1) + add (add may be NULL) and p^2 go through ONE pass over
// the marker-major layout, the per-marker regression test runs in the epilogue: pvals[m] for every local marker (chrom == NULL) or
// for the markers of chromosome ch.  pa / pb: npad doubles of scratch each (they receive p and p^2).
struct PvArgs {
    const uint32_t* cnt;      // 3 per marker: present individuals with a = 2, 1, 0 (marker statistics)
    const double* xself;      // leave-one-out: the marker's own effect x1_hat[m] * self_scale is added back; NULL: none
    double self_scale;
    const int* chrom;         // LOCO: chromosome of every marker, or NULL
    int ch;
    double *beta = nullptr, *se = nullptr, *t = nullptr;   // gv_assoc_*: M device doubles each, all three or none (gv_pvals_*)
};
void marker_pvals(hipStream_t s, const Plan& pl, const double* y, const double* z1, const double* add, const uint32_t* mask2,
                  int64_t npad, const double* mave, const double* msig, double* pa, double* pb, double* red_partial, const PvArgs& a,
                  double* pvals);
// out[M] = data::ATx(p); p has npad entries (zero at NA / pad slots)
// addx != NULL: out = tau * ATx(p) + gam2 * addx, the whole of vamp::lmmse_mult's epilogue (vamp.cpp:1112-1116)
void atx(hipStream_t s, const Plan& pl, const double* p, int64_t npad, const double* mave, const double* msig,
         double inv_sqrt_n, double* red_partial, double* out, const double* addx = nullptr, double tau = 1.0,
         double gam2 = 0.0, const CgHook* cg = nullptr);
// out[npad] = mask * (A~ x) * post   (post = 1/sqrt(N), or 1 when a cross-rank all-reduce follows)
void ax(hipStream_t s, const Plan& pl, const double* x, const double* mave, const double* msig, const uint32_t* mask2,
        int64_t npad, double post, double* red_partial, double* out, const CgHook* cg = nullptr);

// the two stages of ax / ax2, for callers that cut the product into individual-range chunks (row groups [rg0, rg1) of pl.rows_n)
void ax_prep(hipStream_t s, const Plan& pl, const double* xa, const double* xb, const double* mave, const double* msig,
             double* red_partial, const CgHook* cg = nullptr);
void ax_rows(hipStream_t s, const Plan& pl, int nv, int64_t rg0, int64_t rg1, const uint32_t* mask2, int64_t npad, double post,
             double* outa, double* outb, const CgHook* cg = nullptr);

int atx_dot_blocks(const Plan& pl);   // number of block partials of the fused <d, p> (CgHook::dot_part)

// two vectors per pass (the LMMSE and the Onsager CG of one VAMP iteration share the operator, vamp.cpp:593-596,:884)
void atx2(hipStream_t s, const Plan& pl, const double* pa, const double* pb, int64_t npad, const double* mave,
          const double* msig, double inv_sqrt_n, double* red_partial, double* outa, double* outb,
          const double* addxa = nullptr, const double* addxb = nullptr, double tau = 1.0, double gam2 = 0.0,
          const CgHook* cg = nullptr);
void ax_people(hipStream_t s, const Plan& pl, int kind, const double* mave, const double* msig, const uint32_t* mask2,
               int64_t npad, double* red_partial, double* out);
void ax2(hipStream_t s, const Plan& pl, const double* xa, const double* xb, const double* mave, const double* msig,
         const uint32_t* mask2, int64_t npad, double post, double* red_partial, double* outa, double* outb,
         const CgHook* cg = nullptr);

// kernel mode 2 (two-level fixed point, gv_mfma.hip MODE 5 / 6): the same products with ~108 bits below the vector's largest entry
// and exact zeros at missing genotypes, one two-vector-shaped pass each
void ax_wide(hipStream_t s, const Plan& pl, const double* x, const double* mave, const double* msig, const uint32_t* mask2,
             int64_t npad, double post, double* red_partial, double* out);
void atx_wide(hipStream_t s, const Plan& pl, const double* p, int64_t npad, const double* mave, const double* msig, double inv_sqrt_n,
              double* red_partial, double* out, const double* addx = nullptr, double tau = 1.0, double gam2 = 0.0);

}  // namespace gvm

// ---- the fixed-point operand pipeline: one copy for gv_mfma.hip, gv_score.hip and gv_atxm.hip ------------------------------------------
// The batch kernels promise that column j is bit-identical to gv_ax_dev / gv_atx_dev of that column alone; the floating-point steps
// around the exact integer sums -- block partials, the four scalars, the digit split, the limbs -- are these functions in all three
// files, so their roundings and orders agree by construction.  They live here because this file is part of the kernel-source hash
// (build.kernel_src_hash): the streaming kernels compile them in, and a tuning pick or a profile belongs to that hash.
namespace gvm {

constexpr int PREP_STRIDE = 2 * RED_BLOCKS;   // doubles of block partials per vector
// Blocks of a prep launch (every block of the quantisation launch behind it adds their partials up: prep_scalars)
constexpr int PREP_BLOCKS = 256;
inline int prep_blocks(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > PREP_BLOCKS ? PREP_BLOCKS : b));
}
inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

#if defined(__HIPCC__)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// scal[0] = amax, scal[1] = sum (ordered), scal[2] = 2^(54-e) (quantisation multiplier, 0 if amax is 0 / not finite),
// scal[3] = 2^(e-54).  The prep kernels leave block partials; every block of the quantisation launch behind them adds them up
// for itself in a fixed order (prep_scalars: thread t adds blocks t, t + 256, ..., then a binary tree over the 256 threads) and block 0
// stores the four scalars for the epilogue of the pass.  (Until round 3
// the LAST block of the prep launch did it behind a ticket counter: 256 serialised atomics per vector, 12 of the 17-21 us a
// two-vector k_prep_ax took at M = 200k -- profiles/r3_cfg5_gaps.txt.)
__device__ __forceinline__ void prep_scalars(const double* __restrict__ partial, int nblocks, double* shm, double* shs,
                                              double (&out)[4]) {
    double mx = 0.0, s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        mx = fmax(mx, partial[2 * b]);
        s += partial[2 * b + 1];
    }
    shm[threadIdx.x] = mx;
    shs[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            shm[threadIdx.x] = fmax(shm[threadIdx.x], shm[threadIdx.x + off]);
            shs[threadIdx.x] += shs[threadIdx.x + off];
        }
        __syncthreads();
    }
    const double amax = shm[0];
    out[0] = amax;
    out[1] = shs[0];
    if (amax > 0.0 && amax <= 1.7976931348623157e308) {
        int e = ilogb(amax) + 1;
        out[2] = ldexp(1.0, 54 - e);
        out[3] = ldexp(1.0, e - 54);
    } else if (amax == 0.0) {
        out[2] = 0.0;
        out[3] = 0.0;
    } else {
        // a NaN or an infinity among the entries (the prep kernels raise amax to +inf for either): fixed point has no
        // encoding for it.  Defined behaviour = what fp64 sums over the whole vector give in the reference: every
        // output entry of this product is NaN (digits are quantised with multiplier 0, the epilogue multiplies by NaN).
        out[2] = 0.0;
        out[3] = __longlong_as_double(0x7ff8000000000000LL);
    }
}
// block partials of a prep launch of 256 threads: [2b] = max, [2b + 1] = sum (fixed order within the block: wave butterflies, then the
// four wave results in order)
__device__ __forceinline__ void prep_block_partials(double* partial_v, double mx, double s, double* shm, double* shs) {
    mx = wave_max(mx);
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) { shm[threadIdx.x >> 6] = mx; shs[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_v[2 * blockIdx.x] = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
        partial_v[2 * blockIdx.x + 1] = shs[0] + shs[1] + shs[2] + shs[3];
    }
}
// the seven balanced base-256 digits of q into byte t of dig[0..7) (digit column 7 stays zero)
__device__ __forceinline__ void digits_of(long long q, int t, uint32_t (&dig)[8]) {
#pragma unroll
    for (int c = 0; c < 7; c++) {
        long long dg = (long long)(signed char)(q & 0xFF);   // balanced digit in [-128, 127]
        q = (q - dg) >> 8;
        dig[c] |= (uint32_t)(dg & 0xFF) << (8 * t);
    }
}
// exact digit recombination: sum_c s_c 256^c as (hi, lo) with value = hi * 2^32 + lo
__device__ __forceinline__ void combine(const long long (&s)[7], long long& hi, long long& lo) {
    lo = s[0] + (s[1] << 8) + (s[2] << 16) + (s[3] << 24);
    hi = s[4] + (s[5] << 8) + (s[6] << 16);
}

// The two operand planes of four expanded 2-bit codes e (one per byte).  PK 0: r' (the code itself) / missing (1 where the code is 3);
// 1: a^2 (byte LUT r' -> {0,1,4,0}) / missing; 2: a' = a if present else 0 (r' -> {0,1,2,0}) / present (r' -> {1,1,1,0})
template <int PK> __device__ __forceinline__ uint32_t plane_x(uint32_t e) {
    return PK == 0 ? e : __builtin_amdgcn_perm(PK == 1 ? 0x00040100u : 0x00020100u, PK == 1 ? 0x00040100u : 0x00020100u, e);
}
template <int PK> __device__ __forceinline__ uint32_t plane_y(uint32_t e) {
    return __builtin_amdgcn_perm(PK == 2 ? 0x00010101u : 0x01000000u, PK == 2 ? 0x00010101u : 0x01000000u, e);
}

// one workgroup barrier that orders LDS only: the vector-memory prefetches in flight (vmcnt) stay in flight across it
__device__ __forceinline__ void wg_barrier_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// a super-block of the tile layout in registers (gv_mfma.hip, "ONE resident layout for both products"): four 16-byte pieces per lane
struct ABufT { u32x4 t[4]; };

template <int DIR>   // 0: ATx side (rows = markers), 1: Ax side (rows = individuals)
__device__ __forceinline__ void load_t(ABufT& a, const u32x4* __restrict__ sb, int lane) {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int off = (DIR == 0) ? i * 64 + r * 4 + g : (r >> 2) * 64 + (4 * i + g) * 4 + (r & 3);
        a.t[i] = __builtin_nontemporal_load(sb + off);
    }
}
// ATx side: the 4 x 4 byte transpose of the four dwords of a piece, T[t] byte d = byte t of dword d
__device__ __forceinline__ void transpose_piece(const u32x4& p, uint32_t (&T)[4]) {
    const uint32_t L0 = p.x, L1 = p.y, L2 = p.z, L3 = p.w;
    const uint32_t a0 = __builtin_amdgcn_perm(L1, L0, 0x05010400u), a1 = __builtin_amdgcn_perm(L1, L0, 0x07030602u);
    const uint32_t b0 = __builtin_amdgcn_perm(L3, L2, 0x05010400u), b1 = __builtin_amdgcn_perm(L3, L2, 0x07030602u);
    T[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u);
    T[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
    T[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u);
    T[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
}
#endif  // __HIPCC__

}  // namespace gvm
