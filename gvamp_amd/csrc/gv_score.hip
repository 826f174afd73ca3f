// gv_score.hip -- Z = A W for W of M x C columns: many data::Ax products in one pass over the resident genotypes
// (gv_score_dev / gv_score / gv_score_info).
//
// Column j of the result is bit-identical to gv_ax_dev of that column alone.  Where the kernel below does not apply -- two stripe
// sets, kernel modes 0 and 2, methylation and dosage data, a communicator or gv_debug_force_multi, an empty shard -- the existing
// dispatcher (gvi::ax_pass) runs, in pairs and singly: identical by construction.  The kernel is identical because every sum is an
// exact integer and the floating-point steps around it are the functions gv_mfma.hip runs (gv_mfma.h: prep_block_partials,
// prep_scalars, digits_of, combine).  What this file writes itself, in the form of k_prep_ax and k_fin_ax:
//   operands      c = fl(msig x), e = fl(fl(mave - 3) c); a column's scale from max(|c|, |e|)
//   K0            sum of fl(mave c): a grid-stride loop of prep_blocks(M) blocks of 256 threads, each thread's terms in index order
//                 (s += mave * c, contracted to one fma by the compiler as in k_prep_ax)
//   T             fl(fl(hi) * 2^32 + fl(lo)) of the exact (hi, lo) limbs, times the power of two 2^(e-54)
//   out           fl(fl(T - K0) * post) at an individual with a phenotype, an exact 0 elsewhere
// A column with a NaN or an infinity quantises with multiplier 0 and is scaled by NaN: that column is NaN, no other is touched
// (every column has its own digit columns and accumulators).
//
// Tile layout, Ax side (gv_mfma.hip, k_tile_build): super-block (K-step kb of 64 markers, row group rg of 256 individuals) = 4 KiB at
// (kb * nrg + rg) * 4 KiB, 256 pieces of 16 bytes; piece (JB, q_local, J & 3) at JB * 64 + q_local * 4 + (J & 3), dword d of a piece =
// individuals 16 J + 4 d + s (bits 2s of each byte), byte t = marker 4 q_local + t.  The MFMA A operand of row tile (d, s): lane
// (rho = lane & 15, gam = lane >> 4), register i = dword d of piece (q_local = 4 i + gam, J_local = rho) >> 2 s & 0x03030303, i.e. row
// rho = individuals 16 rho + 4 d + s, K-entry 16 i + 4 gam + t.  The B operand of a pair of columns (a, b): lane (col = lane & 15, gam),
// register i byte t = digit col & 7 of column (col >> 3 ? b : a) at marker 16 i + 4 gam + t.
//
// Shape of the work: a workgroup of 4 waves owns 256 individuals x the K-steps of one segment; wave w owns the row tiles d = w, i.e.
// 64 individuals; the workgroup brings a super-block into LDS once and wave w reads dword w of every piece from there.  Per K-step it expands the 2-bit codes into the r' and miss operands ONCE
// (four row tiles) and multiplies them against CP / 2 pairs of digit blocks from LDS: r' . [c_a | c_b] and miss . [e_a | e_b] into the
// SAME accumulator (they are only ever used added): 16 accumulator registers per pair of columns and lane, 8 CP in all.
// Partial sums between the pass and the epilogue are int32 digit planes: 32 bytes per segment, column and row.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "gv_internal.h"
#include "gv_score_plan.h"

// the plan headers are host-only (no HIP include): what they restate of gv_mfma.h is pinned here
static_assert(gvb::MAX_KS == gvm::GV_MAX_KS, "gv_batch_plan.h restates GV_MAX_KS");
static_assert(gvs::ENTRY_MAX == gvm::GV_AX_ENTRY_MAX, "gv_score_plan.h restates the int32 bound of the Ax side");
static_assert(gvb::PREP_BLOCKS_MAX == RED_BLOCKS, "gv_batch_plan.h restates the stride of the preparation's block partials");

namespace {

// the fixed-point operand pipeline, the tile-layout operand helpers and the launch arithmetic: the one copy in gv_mfma.h
using gvm::v4i; using gvm::u32x4; using gvm::PREP_STRIDE; using gvm::prep_blocks; using gvm::nblk; using gvm::prep_block_partials;
using gvm::prep_scalars; using gvm::digits_of; using gvm::combine; using gvm::plane_x; using gvm::plane_y; using gvm::wg_barrier_lds;

struct Cols { const double* x[gvs::CP_MAX]; double* out[gvs::CP_MAX]; };
struct SegB { uint32_t b[gvs::MAX_KS + 1]; };

// ---- preparation: block partials [2b] = max(|c|, |e|), [2b + 1] = sum mave * c of column blockIdx.y (k_prep_ax without its hooks)
__global__ __launch_bounds__(256) void k_score_prep(Cols a, const double* __restrict__ mave, const double* __restrict__ msig, int64_t M,
                                                    double* __restrict__ partial) {
    __shared__ double shm[4], shs[4];
    const int v = blockIdx.y;
    const double* x = a.x[v];
    double mx = 0.0, s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        double xi = x[i];
        double c = msig[i] * xi, mu = mave[i];
        double e = (mu - 3.0) * c;
        mx = (isfinite(c) && isfinite(e)) ? fmax(mx, fmax(fabs(c), fabs(e))) : __longlong_as_double(0x7ff0000000000000LL);
        s += mu * c;
    }
    prep_block_partials(partial + (int64_t)v * PREP_STRIDE, mx, s, shm, shs);
}

// ---- digits of the pass: K-step kstep holds CP / 2 pairs x (c block | e block) x 64 lanes x 16 bytes; dword index
// kstep * CP * 256 + ((pair * 2 + plane) * 64 + gam * 16 + (col & 1) * 8 + digit) * 4 + i  <->  markers 64 kstep + 16 i + 4 gam + t in
// byte t.  blockIdx.y = 2 * column + plane (0: c, 1: e); the columns from ncols on are zero.  Thread = (kstep, i, gam), as k_quant_t.
__global__ __launch_bounds__(256) void k_score_quant(Cols a, const double* __restrict__ mave, const double* __restrict__ msig, int64_t M,
                                                     int64_t nkb, int cp, int ncols, int nblocks, const double* __restrict__ partial,
                                                     double* __restrict__ scal, uint32_t* __restrict__ dig) {
    __shared__ double shm[256], shs[256];
    const int col = blockIdx.y >> 1, plane = blockIdx.y & 1;
    double mult = 0.0;
    if (col < ncols) {
        double sc[4];
        prep_scalars(partial + (int64_t)col * PREP_STRIDE, nblocks, shm, shs, sc);
        if (blockIdx.x == 0 && threadIdx.x == 0 && plane == 0) {
            double* o = scal + 4 * col;
            o[0] = sc[0]; o[1] = sc[1]; o[2] = sc[2]; o[3] = sc[3];
        }
        mult = sc[2];
    }
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= nkb * 16) return;
    const int gam = tid & 3, i = (tid >> 2) & 3;
    const int64_t kstep = tid >> 4;
    uint32_t d8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < ncols) {
        const double* x = a.x[col];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int64_t k = 4 * tid + t;                       // = 64 kstep + 16 i + 4 gam + t
            double val = 0.0;
            if (k < M) {
                const double c = msig[k] * x[k];
                val = plane ? (mave[k] - 3.0) * c : c;
            }
            digits_of((long long)rint(val * mult), t, d8);
        }
    }
    uint32_t* o = dig + kstep * ((int64_t)cp * 256) + (((col >> 1) * 2 + plane) * 64 + gam * 16 + (col & 1) * 8) * 4 + i;
#pragma unroll
    for (int c8 = 0; c8 < 8; c8++) o[c8 * 4] = d8[c8];
}

// ---- the pass.  grid = ks * nrg, item = segment * nrg + row group (segment-major).  partial: [(segment * ncols + column) * rows_p +
// row] * 8 + digit, rows_p = 256 * nrg.
template <int CP>
__global__ __launch_bounds__(256, CP == 16 ? 2 : 3) void k_score(const uint32_t* __restrict__ tiles, const u32x4* __restrict__ dig, int64_t nrg, SegB sb,
                                                  int32_t* __restrict__ partial, int ncols) {
    constexpr int NP = CP / 2;               // pairs of columns
    constexpr int SS = NP * 128;             // u32x4 per LDS stage = per K-step of digits
    constexpr int NC = SS / 256;             // u32x4 a thread moves per K-step
    __shared__ u32x4 sB[2][SS];
    __shared__ u32x4 sA[2][256];             // the super-block of a K-step: read from memory ONCE per workgroup, whole 16-byte pieces
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rho = lane & 15, gam = lane >> 4;
    const int64_t seg = blockIdx.x / nrg, rg = blockIdx.x - seg * nrg;
    const int64_t kb0 = sb.b[seg], nsteps = (int64_t)sb.b[seg + 1] - kb0;
    if (nsteps <= 0) return;                 // (uniform over the workgroup; a plan has no empty segment)
    const int64_t kstride = nrg * 256;       // u32x4 from one K-step to the next
    const u32x4* ap = reinterpret_cast<const u32x4*>(tiles) + (kb0 * nrg + rg) * 256 + tid;
    // dword w of piece (q_local = 4 i + gam, J_local = rho): piece index (rho >> 2) * 64 + (4 i + gam) * 4 + (rho & 3)
    const int aofs = ((rho >> 2) * 64 + gam * 4 + (rho & 3)) * 4 + w;
    const u32x4* dp = dig + kb0 * SS + tid;

    v4i acc[NP][4];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int s = 0; s < 4; s++) acc[p][s] = (v4i){0, 0, 0, 0};

    // genotypes two K-steps ahead (one in registers, one on its way), digits one K-step ahead, both through two-stage LDS rings
    u32x4 rd[NC], ra1, ra2;
#pragma unroll
    for (int j = 0; j < NC; j++) rd[j] = dp[j * 256];
    ra1 = __builtin_nontemporal_load(ap);
#pragma unroll
    for (int j = 0; j < NC; j++) sB[0][tid + j * 256] = rd[j];
    sA[0][tid] = ra1;
    ra1 = __builtin_nontemporal_load(ap + (nsteps > 1 ? kstride : 0));
    wg_barrier_lds();

#pragma unroll 1
    for (int64_t st = 0; st < nsteps; st++) {
        // the last steps fetch the last operands again (no branch in the body)
        const int64_t nx = st + 1 < nsteps ? st + 1 : nsteps - 1, nx2 = st + 2 < nsteps ? st + 2 : nsteps - 1;
#pragma unroll
        for (int j = 0; j < NC; j++) rd[j] = dp[nx * SS + j * 256];
        ra2 = __builtin_nontemporal_load(ap + nx2 * kstride);
        const u32x4* cur = sB[st & 1];
        const uint32_t* acur = reinterpret_cast<const uint32_t*>(sA[st & 1]) + aofs;
        const uint32_t a0 = acur[0], a1 = acur[64], a2 = acur[128], a3 = acur[192];
        v4i X[4], Y[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t e0 = (a0 >> (2 * s)) & 0x03030303u, e1 = (a1 >> (2 * s)) & 0x03030303u, e2 = (a2 >> (2 * s)) & 0x03030303u,
                           e3 = (a3 >> (2 * s)) & 0x03030303u;
            X[s] = (v4i){(int)plane_x<0>(e0), (int)plane_x<0>(e1), (int)plane_x<0>(e2), (int)plane_x<0>(e3)};      // r' plane
            Y[s] = (v4i){(int)plane_y<0>(e0), (int)plane_y<0>(e1), (int)plane_y<0>(e2), (int)plane_y<0>(e3)};      // miss plane
        }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const u32x4 q0 = cur[p * 128 + lane], q1 = cur[p * 128 + 64 + lane];
            const v4i B0 = {(int)q0.x, (int)q0.y, (int)q0.z, (int)q0.w};
            const v4i B1 = {(int)q1.x, (int)q1.y, (int)q1.z, (int)q1.w};
#pragma unroll
            for (int s = 0; s < 4; s++) acc[p][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(X[s], B0, acc[p][s], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; s++) acc[p][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Y[s], B1, acc[p][s], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NC; j++) sB[(st + 1) & 1][tid + j * 256] = rd[j];
        sA[(st + 1) & 1][tid] = ra1;
        wg_barrier_lds();
        ra1 = ra2;
    }

    // D[row 4 gam + reg][col] of row tile (d = w, s): individual 256 rg + 16 (4 gam + reg) + 4 w + s; column 2 p + (col >> 3), digit col & 7
    const int64_t rows_p = nrg * 256;
    const int cd = rho & 7, pv = rho >> 3;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int col = 2 * p + pv;
        if (col >= ncols) continue;
        int32_t* base = partial + ((seg * ncols + col) * rows_p + rg * 256) * 8 + cd;
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) base[(16 * (4 * gam + reg) + 4 * w + s) * 8] = acc[p][s][reg];
    }
}

// ---- epilogue of column blockIdx.y: out[n] = mask (T scale - K0) * post (k_fin_ax)
__global__ __launch_bounds__(256) void k_score_fin(const int32_t* __restrict__ partial, int ks, int ncols, int64_t rows_p, int64_t npad,
                                                   const double* __restrict__ scal_base, const uint32_t* __restrict__ mask2, double post,
                                                   Cols a) {
    const int v = blockIdx.y;
    const double* __restrict__ scal = scal_base + 4 * v;
    double* __restrict__ out = a.out[v];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    double val = 0.0;
    const uint32_t present = (mask2[n >> 4] >> (2 * (n & 15))) & 1u;
    if (present && n < rows_p) {
        long long s[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < ks; k++) {
            const int4* q = reinterpret_cast<const int4*>(partial + (((int64_t)k * ncols + v) * rows_p + n) * 8);
            const int4 x0 = q[0], x1 = q[1];
            s[0] += x0.x; s[1] += x0.y; s[2] += x0.z; s[3] += x0.w;
            s[4] += x1.x; s[5] += x1.y; s[6] += x1.z;
        }
        long long xh, xl;
        combine(s, xh, xl);
        const double T = ((double)xh * 4294967296.0 + (double)xl) * scal[3];
        val = (T - scal[1]) * post;
    }
    out[n] = val;
}

template <int CP>
void launch_pass(hipStream_t s, const gv_ctx* c, const gvs::Plan& p, const SegB& sb, const u32x4* dig, int32_t* part, int ncols) {
    hipLaunchKernelGGL(k_score<CP>, dim3((unsigned)p.items), dim3(256), 0, s, (const uint32_t*)c->plan.tiles, dig, p.nrg, sb, part, ncols);
}

}  // namespace

namespace gvi {

// the kernel applies: kernel mode 1 on the tile layout, 2-bit genotypes, one rank, a shard with markers
static bool score_kernel_applies(const gv_ctx* c) {
    return !c->dense.resident && c->kernel_mode == 1 && c->have_stripes && c->plan.layout == 1 && c->plan.tiles && !is_multi(c) && c->M > 0;
}

static int score_kernel(gv_ctx* c, int64_t C, const double* const* x, double* const* out, gv_score_stats& st) {
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int cp0 = c->score_cols ? c->score_cols : GV_SCORE_COLS_DEFAULT;
    const gvs::Plan p = gvs::make_plan(c->N, c->M, C, cp0, c->score_ks, 24 * (int64_t)(cus > 0 ? cus : 256));
    if (p.err == 1)
        return fail(c, "gv_score_dev: GV_SCORE_KS=%d: a K-segment of %lld markers would let an int32 digit sum wrap (at most %lld markers "
                       "per segment; this shard of %lld markers needs at least %d segments)", c->score_ks,
                    (long long)gvs::longest_segment(p.nkb, p.ks, c->M), (long long)gvs::SEG_MARKERS_MAX, (long long)c->M, p.min_ks);
    if (p.err)
        return fail(c, "gv_score_dev: a shard of %lld markers cannot be split into at most %d K-segments of at most %lld markers",
                    (long long)c->M, gvs::MAX_KS, (long long)gvs::SEG_MARKERS_MAX);
    // the same question put to the project's own bound (equal segments of make_bounds) and its floor
    gvm::Decomp d;
    d.ks = p.ks;
    const int floor_ks = gvm::ax_min_ks(p.nkb, 64, c->M);
    if (floor_ks <= 0 || p.ks < floor_ks || !gvm::ax_bound_ok(d, p.nkb, 64, c->M))
        return fail(c, "gv_score_dev: %d K-segments do not keep the int32 bound of the Ax side on this shard of %lld markers (at least %d)",
                    p.ks, (long long)c->M, floor_ks);
    if (p.nrg != c->plan.nrg_n || p.nkb != c->plan.nkb_n)
        return fail(c, "gv_score_dev: the resident tile layout has %lld x %lld super-blocks, the plan %lld x %lld", (long long)c->plan.nrg_n,
                    (long long)c->plan.nkb_n, (long long)p.nrg, (long long)p.nkb);
    if (!c->score_scratch.reserve(p.scratch_bytes))
        return fail(c, "gv_score_dev: cannot allocate %zu bytes of scratch (digits %zu, partial sums %zu)", p.scratch_bytes, p.dig_bytes,
                    p.part_bytes);
    char* buf = static_cast<char*>(c->score_scratch.buf);
    u32x4* dig = reinterpret_cast<u32x4*>(buf);
    int32_t* part = reinterpret_cast<int32_t*>(buf + p.dig_bytes);
    double* scal = reinterpret_cast<double*>(buf + p.dig_bytes + p.part_bytes);
    double* prep = scal + 4 * p.cp;
    SegB sb;
    memcpy(sb.b, p.b, sizeof(sb.b));
    const int nb = prep_blocks(c->M);
    const double post = 1.0 / sqrt((double)c->N);
    hipStream_t s = c->stream;
    for (int64_t ps = 0; ps < p.passes; ps++) {
        const int ncols = (int)gvs::pass_cols(ps, C, p.cp);
        const int cp = ps == p.passes - 1 ? p.cp_last : p.cp;
        Cols cl{};
        for (int j = 0; j < ncols; j++) { cl.x[j] = x[ps * p.cp + j]; cl.out[j] = out[ps * p.cp + j]; }
        hipLaunchKernelGGL(k_score_prep, dim3(nb, ncols), dim3(256), 0, s, cl, c->mave, c->msig, c->M, prep);
        hipLaunchKernelGGL(k_score_quant, dim3(nblk(p.nkb * 16, 256), 2 * cp), dim3(256), 0, s, cl, c->mave, c->msig, c->M, p.nkb, cp, ncols,
                           nb, prep, scal, reinterpret_cast<uint32_t*>(dig));
        if (cp == 4) launch_pass<4>(s, c, p, sb, dig, part, ncols);
        else if (cp == 8) launch_pass<8>(s, c, p, sb, dig, part, ncols);
        else launch_pass<16>(s, c, p, sb, dig, part, ncols);
        hipLaunchKernelGGL(k_score_fin, dim3(nblk(c->npad, 256), ncols), dim3(256), 0, s, part, p.ks, ncols, p.nrg * 256, c->npad, scal,
                           c->mask2, post, cl);
        KCHK(c);
    }
    c->cnt.n_ax += C;
    c->cnt.n_ax_pass += p.passes;
    st.path = GV_SCORE_PATH_KERNEL;
    st.cols_per_pass = p.cp;
    st.passes = p.passes;
    st.ksegs = p.ks;
    st.scratch_bytes = p.scratch_bytes;
    return 0;
}

int score_device(gv_ctx* c, int64_t C, const double* const* x, double* const* out) {
    const auto t0 = std::chrono::steady_clock::now();
    gv_score_stats st{};
    st.columns = C;
    st.min_cols = c->score_min_cols;
    const bool kernel = score_kernel_applies(c) && C >= c->score_min_cols;
    if (kernel) {
        NEED(c, c->have_stats && c->mask2, "Ax: bed, mask and marker statistics must be set first");
        if (score_kernel(c, C, x, out, st)) return 1;
    } else {
        if (ensure_work(c)) return 1;
        const int64_t pass0 = c->cnt.n_ax_pass;
        int64_t j = 0;
        for (; j + 2 <= C; j += 2)
            if (ax_pass(c, 2, x[j], x[j + 1], out[j], out[j + 1], nullptr)) return 1;
        if (j < C && ax_pass(c, 1, x[j], nullptr, out[j], nullptr, nullptr)) return 1;
        st.path = GV_SCORE_PATH_FALLBACK;
        st.passes = c->cnt.n_ax_pass - pass0;
        st.cols_per_pass = st.passes * 2 <= C + 1 ? 2 : 1;
    }
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->score_last = st;
    return 0;
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_score_dev(gv_ctx* c, int64_t C, const gv_vec* const* x, gv_vec* const* out) {
    NEED(c, C >= 0, "gv_score_dev: the number of columns is negative");
    if (C == 0) return 0;
    NEED(c, x && out, "gv_score_dev: the arrays of column handles are NULL");
    std::vector<const double*> xs;
    std::vector<double*> os;
    if (batch_args(c, "gv_score_dev", C, x, out, "x", GV_SPACE_M, xs, os)) return 1;
    return score_device(c, C, xs.data(), os.data());
}

int gv_score(gv_ctx* c, int64_t C, const double* W, double* out) {
    NEED(c, C >= 0, "gv_score: the number of columns is negative");
    if (C == 0) return 0;
    NEED(c, W && out, "gv_score: W or out is NULL");
    return batch_host(c, "gv_score", C, W, GV_SPACE_M, false, out, gv_score_dev, &c->score_last.seconds);
}

int gv_score_info(const gv_ctx* c, gv_score_stats* out) {
    if (!c || !out) return 1;
    *out = c->score_last;
    out->min_cols = c->score_min_cols;
    return 0;
}

}  // extern "C"
