// gv_atxm.hip -- R = A^T Y for Y of N x C columns: many data::ATx products in one pass over the resident genotypes
// (gv_atxm_dev / gv_atxm / gv_atxm_info), and the marginal association screen on it (gv_screen_dev); DESIGN.md section 23.
//
// Column j of the result is bit-identical to gv_atx_dev of that column alone.  Where the kernel below does not apply -- two stripe
// sets, kernel modes 0 and 2, methylation and dosage data, an empty shard, fewer columns than min_cols -- the existing dispatcher
// (gvi::atx_pass) runs, in pairs and singly: identical by construction.  8-bit dosage codes on the fixed-point route have a kernel of
// their own (gv_dense_atxm.hip; atxm_dense_kernel below), with the same contract.  (ATx issues no collective, so a communicator or
// gv_debug_force_multi does not disqualify the kernel.)  The kernel is identical because every sum is an exact integer and the
// floating-point steps around it are the functions gv_mfma.hip runs (gv_mfma.h: prep_block_partials, prep_scalars, digits_of,
// combine).  What this file writes itself, in the form of k_prep_atx (without its CG hook) and k_fin_atx (without addx):
//   scale, P      max |p| (raised to +inf by a NaN or an infinity) and P = sum p over all npad slots: a grid-stride loop of
//                 prep_blocks(npad) blocks of 256 threads, each thread's terms in index order (s += val).  Both depend on npad alone.
//   planes        X = sum r' digit, Y = sum miss digit per marker, kept apart: the epilogue scales them differently
//   epilogue      (hi, lo) limbs of each plane; sa = fl(fl(fl(xh - 3 yh) 2^32 + fl(xl - 3 yl)) scale),
//                 sm = fl(fl(fl(yh) 2^32 + fl(yl)) scale), out = fl(fl(msig fma(-mave, fl(P - sm), sa)) / sqrt(N))
// A column with a NaN or an infinity quantises with multiplier 0 and is scaled by NaN: that column is NaN, no other is touched
// (every column has its own digit columns and accumulators).
//
// Tile layout, ATx side (gv_mfma.hip, k_tile_build): super-block (marker group rg of 64 markers, K-step kb of 256 individuals) = 4 KiB
// at (rg * nkb + kb) * 4 KiB, 256 pieces of 16 bytes; load i of a wave: lane (r, g) takes piece i * 64 + r * 4 + g = marker quad r,
// individuals 256 kb + 64 i + 16 g ..; a 4 x 4 byte transpose of its four dwords gives T[t] = marker 4 r + t, byte d <-> individuals
// + 4 d + s at bit pair s.  The MFMA A operand of row tile t: register s = (T[t] >> 2 s) & 0x03030303, i.e. row r = marker 64 rg + 4 r
// + t, K-entry 64 i + 16 g + 4 d + s.  The B operand of a pair of columns (a, b): lane (c, g), load i: the 16-byte element
// g * 64 + i * 16 + c of the pair's block, register s byte d = digit c & 7 of column (c >> 3 ? b : a) at that K-entry (k_quant's order).
//
// Shape of the work: a workgroup of 4 waves owns 4 consecutive marker groups x the K-steps of one segment; each wave streams its own
// super-blocks (four 16-byte non-temporal loads per K-step, two K-steps in flight), the workgroup brings the digit block of a K-step
// -- 2 KiB per column -- into LDS once through a two-stage ring.  Per load a wave transposes and expands the 2-bit codes into the r'
// and miss operands ONCE (four row tiles) and multiplies them against CP / 2 pairs of digit columns: 8 accumulator registers per tile
// and pair, 16 CP in all.  Partial sums between the pass and the epilogue are int32 digit planes: 64 bytes per segment, column and
// marker.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gv_internal.h"
#include "gv_atxm_plan.h"
#include "gv_dense_atxm_plan.h"
#include "gv_pval_dev.h"

namespace {

// the fixed-point operand pipeline, the tile-layout operand helpers and the launch arithmetic: the one copy in gv_mfma.h
using gvm::v4i; using gvm::u32x4; using gvm::PREP_STRIDE; using gvm::prep_blocks; using gvm::nblk; using gvm::prep_block_partials;
using gvm::prep_scalars; using gvm::digits_of; using gvm::combine; using gvm::plane_x; using gvm::plane_y; using gvm::wg_barrier_lds;
using gvm::ABufT; using gvm::transpose_piece;

struct Cols { const double* p[gvx::CP_MAX]; double* out[gvx::CP_MAX]; };
struct SegB { uint32_t b[gvx::MAX_KS + 1]; };

// ---- preparation: block partials [2b] = max |p|, [2b + 1] = sum p of column blockIdx.y (k_prep_atx without its hook)
__global__ __launch_bounds__(256) void k_atxm_prep(Cols a, int64_t n, double* __restrict__ partial) {
    __shared__ double shm[4], shs[4];
    const int v = blockIdx.y;
    const double* p = a.p[v];
    double mx = 0.0, s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double val = p[i];
        mx = isfinite(val) ? fmax(mx, fabs(val)) : __longlong_as_double(0x7ff0000000000000LL);   // fmax would drop a NaN
        s += val;
    }
    prep_block_partials(partial + (int64_t)v * PREP_STRIDE, mx, s, shm, shs);
}

// ---- digits of the pass: K-step kb holds CP / 2 pairs x 256 elements of 16 bytes; dword index
// kb * CP * 512 + (col >> 1) * 1024 + d * 256 + g * 64 + ((col & 1) * 8 + digit) * 4 + s  <->  individuals 256 kb + 64 g + 16 d + 4 t + s in
// byte t (k_quant with 16 columns per pair).  blockIdx.y = column; the columns from ncols on are zero.  Thread = (kb, g, d, s).
__global__ __launch_bounds__(256) void k_atxm_quant(Cols a, int64_t n, int64_t nkb, int cp, int ncols, int nblocks,
                                                    const double* __restrict__ partial, double* __restrict__ scal, uint32_t* __restrict__ dig) {
    __shared__ double shm[256], shs[256];
    const int col = blockIdx.y;
    double mult = 0.0;
    if (col < ncols) {
        double sc[4];
        prep_scalars(partial + (int64_t)col * PREP_STRIDE, nblocks, shm, shs, sc);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            double* o = scal + 4 * col;
            o[0] = sc[0]; o[1] = sc[1]; o[2] = sc[2]; o[3] = sc[3];
        }
        mult = sc[2];
    }
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= nkb * 64) return;
    const int s = tid & 3, d = (tid >> 2) & 3, g = (tid >> 4) & 3;
    const int64_t kb = tid >> 6;
    uint32_t d8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < ncols) {
        const double* v = a.p[col];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int64_t k = kb * 256 + 64 * g + 16 * d + 4 * t + s;
            const double val = (k < n) ? v[k] : 0.0;
            digits_of((long long)rint(val * mult), t, d8);
        }
    }
    uint32_t* o = dig + kb * ((int64_t)cp * 512) + (col >> 1) * 1024 + d * 256 + g * 64 + (col & 1) * 32 + s;
#pragma unroll
    for (int c8 = 0; c8 < 8; c8++) o[c8 * 4] = d8[c8];
}

// the four 16-byte non-temporal loads of a super-block, ATx side: the pieces of gvm::load_t<0>.  It stays a function of this file for
// the form of its address alone -- pointer steps, where load_t adds the offsets up as one int first -- which the compiler turns into
// other address arithmetic in the pass kernel; k_atxm's instruction stream is held to the one it was measured with
__device__ __forceinline__ void load_sb(ABufT& a, const u32x4* __restrict__ sb, int lane) {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) a.t[i] = __builtin_nontemporal_load(sb + i * 64 + r * 4 + g);
}

// one K-step of a wave: per load the byte transpose and the plane expansion once, then NP pairs of MFMAs per tile and plane
template <int NP>
__device__ __forceinline__ void compute_step(const ABufT& a, const u32x4* sb, int lane, v4i (&accX)[NP][4], v4i (&accY)[NP][4]) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        v4i B[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const u32x4 bq = sb[p * 256 + g * 64 + i * 16 + c];
            B[p] = (v4i){(int)bq.x, (int)bq.y, (int)bq.z, (int)bq.w};
        }
        uint32_t T[4];
        transpose_piece(a.t[i], T);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t w = T[t];
            const uint32_t e0 = w & 0x03030303u, e1 = (w >> 2) & 0x03030303u, e2 = (w >> 4) & 0x03030303u, e3 = (w >> 6) & 0x03030303u;
            const v4i X = {(int)plane_x<0>(e0), (int)plane_x<0>(e1), (int)plane_x<0>(e2), (int)plane_x<0>(e3)};      // r' plane
            const v4i Y = {(int)plane_y<0>(e0), (int)plane_y<0>(e1), (int)plane_y<0>(e2), (int)plane_y<0>(e3)};      // miss plane
#pragma unroll
            for (int p = 0; p < NP; p++) {
                accX[p][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(X, B[p], accX[p][t], 0, 0, 0);
                accY[p][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Y, B[p], accY[p][t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- the pass.  grid = ks * nq, item = segment * nq + quad (segment-major, dealt by block index).  partial:
// [(((segment * ncols + column) * rows_p + marker) * 2 + plane) * 8 + digit], rows_p = 64 * nrg, plane 0 = X, 1 = Y.
template <int CP>
__global__ __launch_bounds__(256, 2) void k_atxm(const u32x4* __restrict__ tiles, const u32x4* __restrict__ dig, int64_t nrg,
                                                               int64_t nkb, int64_t nq, SegB sb, int32_t* __restrict__ partial, int ncols) {
    constexpr int NP = CP / 2;               // pairs of columns
    constexpr int SS = NP * 256;             // u32x4 per LDS stage = per K-step of digits
    __shared__ u32x4 sB[2][SS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t seg = blockIdx.x / nq, quad = blockIdx.x - seg * nq;
    const int64_t kb0 = sb.b[seg], nsteps = (int64_t)sb.b[seg + 1] - kb0;
    if (nsteps <= 0) return;                 // (uniform over the workgroup; a plan has no empty segment)
    int64_t rg = quad * 4 + w;
    const bool live = rg < nrg;              // a wave past the last marker group streams the last one again and stores nothing
    if (!live) rg = nrg - 1;
    const u32x4* ap = tiles + (rg * nkb + kb0) * 256;
    const u32x4* dp = dig + kb0 * SS + tid;
    const int64_t last = nsteps - 1;

    v4i accX[NP][4], accY[NP][4];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            accX[p][t] = (v4i){0, 0, 0, 0};
            accY[p][t] = (v4i){0, 0, 0, 0};
        }

    // genotypes two K-steps ahead in three register buffers rotating by name, digits one K-step ahead through a two-stage LDS ring;
    // the last steps fetch the last operands again (no branch in the body)
    ABufT a0, a1, a2;
    u32x4 rd[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) rd[j] = dp[j * 256];
    load_sb(a0, ap, lane);
    load_sb(a1, ap + (last >= 1 ? 256 : 0), lane);
#pragma unroll
    for (int j = 0; j < NP; j++) sB[0][tid + j * 256] = rd[j];
    wg_barrier_lds();
#define GV_X_STEP(CUR, NXT, S)                                                           \
    {                                                                                    \
        const int64_t sv = (S);                                                          \
        const int64_t n1 = sv + 1 < last ? sv + 1 : last, n2 = sv + 2 < last ? sv + 2 : last; \
        _Pragma("unroll") for (int j = 0; j < NP; j++) rd[j] = dp[n1 * SS + j * 256];    \
        load_sb(NXT, ap + n2 * 256, lane);                                               \
        compute_step<NP>(CUR, sB[sv & 1], lane, accX, accY);                             \
        _Pragma("unroll") for (int j = 0; j < NP; j++) sB[(sv + 1) & 1][tid + j * 256] = rd[j]; \
        wg_barrier_lds();                                                                \
    }
    int64_t st = 0;
    const int64_t rem = nsteps % 3;
#pragma unroll 1
    for (; st < rem; st++) {
        GV_X_STEP(a0, a2, st)
        a0 = a1;
        a1 = a2;
    }
#pragma unroll 1
    for (; st < nsteps; st += 3) {
        GV_X_STEP(a0, a2, st)
        GV_X_STEP(a1, a0, st + 1)
        GV_X_STEP(a2, a1, st + 2)
    }
#undef GV_X_STEP
    if (!live) return;

    // tile t: D[row 4 g + reg][col c] <-> marker 64 rg + 4 (4 g + reg) + t; column 2 p + (c >> 3), digit c & 7
    const int64_t rows_p = nrg * 64;
    const int cd = c & 7, pv = c >> 3;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int col = 2 * p + pv;
        if (col >= ncols) continue;
        int32_t* base = partial + ((seg * ncols + col) * rows_p + rg * 64) * 16 + cd;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                int32_t* o = base + (4 * (4 * g + reg) + t) * 16;
                o[0] = accX[p][t][reg];
                o[8] = accY[p][t][reg];
            }
    }
}

// ---- epilogue of column blockIdx.y: out[m] = msig (sum a p - mave sum b p) / sqrt(N) (k_fin_atx without addx)
__global__ __launch_bounds__(256) void k_atxm_fin(const int32_t* __restrict__ partial, int ks, int ncols, int64_t rows_p, int64_t M,
                                                  const double* __restrict__ scal_base, const double* __restrict__ mave,
                                                  const double* __restrict__ msig, double inv_sqrt_n, Cols a) {
    const int v = blockIdx.y;
    const double* __restrict__ scal = scal_base + 4 * v;
    double* __restrict__ out = a.out[v];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long long sx[7] = {0, 0, 0, 0, 0, 0, 0}, sy[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < ks; k++) {
        const int4* q = reinterpret_cast<const int4*>(partial + (((int64_t)k * ncols + v) * rows_p + m) * 16);
        const int4 x0 = q[0], x1 = q[1], y0 = q[2], y1 = q[3];
        sx[0] += x0.x; sx[1] += x0.y; sx[2] += x0.z; sx[3] += x0.w;
        sx[4] += x1.x; sx[5] += x1.y; sx[6] += x1.z;
        sy[0] += y0.x; sy[1] += y0.y; sy[2] += y0.z; sy[3] += y0.w;
        sy[4] += y1.x; sy[5] += y1.y; sy[6] += y1.z;
    }
    long long xh, xl, yh, yl;
    combine(sx, xh, xl);
    combine(sy, yh, yl);
    const double scale = scal[3], P = scal[1];
    // P - sm is written the way the compiler contracts it in k_fin_atx, fma(-scale, Y, P): the product by the power of two is exact, so
    // this is fl(P - sm) bit for bit, and with a NaN scale (a column with a NaN or an infinity) the NaN that comes out has the sign and
    // the payload k_fin_atx gives it
    const double sa = scale * ((double)(xh - 3 * yh) * 4294967296.0 + (double)(xl - 3 * yl));
    const double pm = fma(-scale, (double)yh * 4294967296.0 + (double)yl, P);
    out[m] = msig[m] * fma(-mave[m], pm, sa) * inv_sqrt_n;
}

// ---- the screen's element-wise epilogue of column blockIdx.y (gvamp.h: the rounding sequence of r and t)
struct ScreenCols { double* r[gvx::CP_MAX]; double* t[gvx::CP_MAX]; double* p[gvx::CP_MAX]; };
// qss != NULL (dosage codes, gv_set_screen_dosage): the marker's q = sum ((b - mu') na)^2 of the statistics pass, exact zero for a
// constant or all-missing marker, takes the place of the genotype counts
__global__ __launch_bounds__(256) void k_screen_fin(ScreenCols a, int64_t M, const uint32_t* __restrict__ cnt, const double* __restrict__ mave,
                                                    const double* __restrict__ msig, const double* __restrict__ qss, double rfac, double nu) {
    const int v = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double sumsqx;
    if (qss) {
        sumsqx = qss[m];
    } else {
        // no variance among the phenotyped present genotypes: sumsqx of gvp::marker_stats, in its expression
        const double n2 = cnt[3 * m], n1 = cnt[3 * m + 1], n0 = cnt[3 * m + 2], mu = mave[m], sg = msig[m];
        sumsqx = sg * sg * (n2 * (2.0 - mu) * (2.0 - mu) + n1 * (1.0 - mu) * (1.0 - mu) + n0 * mu * mu);
    }
    double r, t, p;
    if (sumsqx == 0.0) {
        r = t = p = NAN;
    } else {
        r = a.r[v][m] * rfac;
        const double om = fma(-r, r, 1.0);
        if (isnan(r)) {
            t = p = NAN;
        } else if (om <= 0.0) {
            t = copysign(__longlong_as_double(0x7ff0000000000000LL), r);
            p = 0.0;
        } else {
            t = r * sqrt(nu / om);
            p = gvp::t_two_sided(fabs(t), nu);
        }
    }
    a.r[v][m] = r;
    if (a.t[v]) a.t[v][m] = t;
    if (a.p[v]) a.p[v][m] = p;
}

template <int CP>
void launch_pass(hipStream_t s, const gv_ctx* c, const gvx::Plan& p, const SegB& sb, const u32x4* dig, int32_t* part, int ncols) {
    hipLaunchKernelGGL(k_atxm<CP>, dim3((unsigned)p.items), dim3(256), 0, s, (const u32x4*)c->plan.tiles, dig, p.nrg, p.nkb, p.nq, sb, part,
                       ncols);
}

}  // namespace

namespace gvi {

// the kernel applies: kernel mode 1 on the tile layout, 2-bit genotypes, a shard with markers (ATx issues no collective: any rank count)
static bool atxm_kernel_applies(const gv_ctx* c) {
    return !c->dense.resident && c->kernel_mode == 1 && c->have_stripes && c->plan.layout == 1 && c->plan.tiles && c->M > 0;
}

static int atxm_kernel(gv_ctx* c, int64_t C, const double* const* p, double* const* out, gv_atxm_stats& st) {
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int cp0 = c->atxm_cols ? c->atxm_cols : GV_ATXM_COLS_DEFAULT;
    const gvx::Plan pl = gvx::make_plan(c->N, c->M, C, cp0, c->atxm_ks, 24 * (int64_t)(cus > 0 ? cus : 256));
    if (pl.err == 2)
        return fail(c, "gv_atxm_dev: %lld individuals would let an int32 digit sum wrap (at most %lld)", (long long)c->N,
                    (long long)gvx::SEG_INDIVIDUALS_MAX);
    if (pl.err) return fail(c, "gv_atxm_dev: no plan for N = %lld, M = %lld, C = %lld", (long long)c->N, (long long)c->M, (long long)C);
    if (pl.nrg != c->plan.nrg_m || pl.nkb != c->plan.nkb_m)
        return fail(c, "gv_atxm_dev: the resident tile layout has %lld x %lld super-blocks, the plan %lld x %lld", (long long)c->plan.nrg_m,
                    (long long)c->plan.nkb_m, (long long)pl.nrg, (long long)pl.nkb);
    if (!c->atxm_scratch.reserve(pl.scratch_bytes))
        return fail(c, "gv_atxm_dev: cannot allocate %zu bytes of scratch (digits %zu, partial sums %zu)", pl.scratch_bytes, pl.dig_bytes,
                    pl.part_bytes);
    char* buf = static_cast<char*>(c->atxm_scratch.buf);
    u32x4* dig = reinterpret_cast<u32x4*>(buf);
    int32_t* part = reinterpret_cast<int32_t*>(buf + pl.dig_bytes);
    double* scal = reinterpret_cast<double*>(buf + pl.dig_bytes + pl.part_bytes);
    double* prep = scal + 4 * pl.cp;
    SegB sb;
    memcpy(sb.b, pl.b, sizeof(sb.b));
    const int nb = prep_blocks(c->npad);
    const double inv_sqrt_n = 1.0 / sqrt((double)c->N);
    hipStream_t s = c->stream;
    for (int64_t ps = 0; ps < pl.passes; ps++) {
        const int ncols = (int)gvx::pass_cols(ps, C, pl.cp);
        const int cp = ps == pl.passes - 1 ? pl.cp_last : pl.cp;
        Cols cl{};
        for (int j = 0; j < ncols; j++) { cl.p[j] = p[ps * pl.cp + j]; cl.out[j] = out[ps * pl.cp + j]; }
        hipLaunchKernelGGL(k_atxm_prep, dim3(nb, ncols), dim3(256), 0, s, cl, c->npad, prep);
        hipLaunchKernelGGL(k_atxm_quant, dim3(nblk(pl.nkb * 64, 256), cp), dim3(256), 0, s, cl, c->npad, pl.nkb, cp, ncols, nb, prep, scal,
                           reinterpret_cast<uint32_t*>(dig));
        if (cp == 4) launch_pass<4>(s, c, pl, sb, dig, part, ncols);
        else launch_pass<8>(s, c, pl, sb, dig, part, ncols);
        hipLaunchKernelGGL(k_atxm_fin, dim3(nblk(c->M, 256), ncols), dim3(256), 0, s, part, pl.ks, ncols, pl.nrg * 64, c->M, scal, c->mave,
                           c->msig, inv_sqrt_n, cl);
        KCHK(c);
    }
    c->cnt.n_atx += C;
    c->cnt.n_atx_pass += pl.passes;
    st.path = GV_ATXM_PATH_KERNEL;
    st.cols_per_pass = pl.cp;
    st.passes = pl.passes;
    st.ksegs = pl.ks;
    st.scratch_bytes = pl.scratch_bytes;
    return 0;
}

// 8-bit dosage codes while the fixed-point route is in force (the plain kernels: no reserved code in the shard), a shard with markers
static bool atxm_dense_kernel_applies(const gv_ctx* c) { return dosage_mfma_route(c) && c->M > 0; }

static int atxm_dense_kernel(gv_ctx* c, int64_t C, const double* const* p, double* const* out, gv_atxm_stats& st) {
    const int cp0 = c->atxm_cols ? c->atxm_cols : GV_ATXM_DENSE_COLS_DEFAULT;
    const gvdx::Plan pl = gvdx::make_plan(c->N, c->M, C, cp0, c->dosage_seg, c->dense.cus);
    if (pl.err) return fail(c, "gv_atxm_dev: no plan for N = %lld, M = %lld, C = %lld", (long long)c->N, (long long)c->M, (long long)C);
    const gvdm::Shape sh = gvdm::atx_shape(c->N, c->M, c->dense.cus, c->dosage_seg);
    if (sh.segs != pl.cut.segs || sh.seg_steps != pl.cut.seg_steps || sh.steps != pl.cut.steps || sh.blocks != pl.blocks)
        return fail(c, "gv_atxm_dev: the plan cuts %d segments of %lld steps, the one-vector product %d of %lld", pl.cut.segs,
                    (long long)pl.cut.seg_steps, sh.segs, (long long)sh.seg_steps);
    if (!c->atxm_scratch.reserve(pl.scratch_bytes))
        return fail(c, "gv_atxm_dev: cannot allocate %zu bytes of scratch (digits %zu, partial sums %zu)", pl.scratch_bytes, pl.dig_bytes,
                    pl.part_bytes);
    char* buf = static_cast<char*>(c->atxm_scratch.buf);
    int32_t* part = reinterpret_cast<int32_t*>(buf + pl.dig_bytes);
    char* small = buf + pl.dig_bytes + pl.part_bytes;
    const gvd::View v = dense_view(c);
    const double scale = 1.0 / sqrt((double)c->N);
    for (int64_t ps = 0; ps < pl.passes; ps++) {
        const int ncols = (int)gvdx::pass_cols(ps, C, pl.cp);
        const int cp = ps == pl.passes - 1 ? pl.cp_last : pl.cp;
        HIPCHK(c, gvdm::atxm_pass(c->stream, v, sh, cp, c->atxm_dense_tiles, ncols, p + ps * pl.cp, out + ps * pl.cp, scale, buf, pl.pair_dig_bytes, part, small,
                                  pl.pair_small_bytes));
        KCHK(c);
    }
    c->cnt.n_atx += C;
    c->cnt.n_atx_pass += pl.passes;
    st.path = GV_ATXM_PATH_KERNEL;
    st.cols_per_pass = pl.cp;
    st.passes = pl.passes;
    st.ksegs = sh.segs;
    st.scratch_bytes = pl.scratch_bytes;
    return 0;
}

int atxm_device(gv_ctx* c, int64_t C, const double* const* p, double* const* out) {
    const auto t0 = std::chrono::steady_clock::now();
    gv_atxm_stats st{};
    st.columns = C;
    const bool dense_kernel = atxm_dense_kernel_applies(c) && C >= c->atxm_dense_min_cols;
    st.min_cols = atxm_dense_kernel_applies(c) ? c->atxm_dense_min_cols : c->atxm_min_cols;
    const bool kernel = atxm_kernel_applies(c) && C >= c->atxm_min_cols;
    if (dense_kernel) {
        NEED(c, c->have_stats, "ATx: bed and marker statistics must be set first");
        if (atxm_dense_kernel(c, C, p, out, st)) return 1;
    } else if (kernel) {
        NEED(c, c->have_stats, "ATx: bed and marker statistics must be set first");
        if (atxm_kernel(c, C, p, out, st)) return 1;
    } else {
        const int64_t pass0 = c->cnt.n_atx_pass;
        int64_t j = 0;
        for (; j + 2 <= C; j += 2)
            if (atx_pass(c, 2, p[j], p[j + 1], out[j], out[j + 1], nullptr, nullptr, 0.0, 0.0, nullptr)) return 1;
        if (j < C && atx_pass(c, 1, p[j], nullptr, out[j], nullptr, nullptr, nullptr, 0.0, 0.0, nullptr)) return 1;
        st.path = GV_ATXM_PATH_FALLBACK;
        st.passes = c->cnt.n_atx_pass - pass0;
        st.cols_per_pass = st.passes * 2 <= C + 1 ? 2 : 1;
    }
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->atxm_last = st;
    return 0;
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_atxm_dev(gv_ctx* c, int64_t C, const gv_vec* const* p, gv_vec* const* out) {
    NEED(c, C >= 0, "gv_atxm_dev: the number of columns is negative");
    if (C == 0) return 0;
    NEED(c, p && out, "gv_atxm_dev: the arrays of column handles are NULL");
    std::vector<const double*> ps;
    std::vector<double*> os;
    if (batch_args(c, "gv_atxm_dev", C, p, out, "p", GV_SPACE_N, ps, os)) return 1;
    return atxm_device(c, C, ps.data(), os.data());
}

int gv_atxm(gv_ctx* c, int64_t C, const double* Y, double* out) {
    NEED(c, C >= 0, "gv_atxm: the number of columns is negative");
    if (C == 0) return 0;
    NEED(c, Y && out, "gv_atxm: Y or out is NULL");
    NEED(c, c->mask2, "gv_atxm: the phenotype mask must be set first");
    // the staged copies are masked as gv_atx masks its own (a no-op for a filtered column; methylation data: used as given)
    return batch_host(c, "gv_atxm", C, Y, GV_SPACE_N, !c->dense.resident, out, gv_atxm_dev, &c->atxm_last.seconds);
}

int gv_atxm_info(const gv_ctx* c, gv_atxm_stats* out) {
    if (!c || !out) return 1;
    *out = c->atxm_last;
    out->min_cols = atxm_dense_kernel_applies(c) ? c->atxm_dense_min_cols : c->atxm_min_cols;
    return 0;
}

int gv_set_screen_dosage(gv_ctx* c, int on) {
    NEED(c, on == 0 || on == 1, "gv_set_screen_dosage: on must be 0 or 1");
    c->screen_dosage = on;
    return 0;
}

int gv_get_screen_dosage(const gv_ctx* c, int* on) {
    if (!c) return 1;
    if (on) *on = c->screen_dosage;
    return 0;
}

int gv_screen_dev(gv_ctx* c, int64_t C, const gv_vec* const* u, gv_vec* const* r, gv_vec* const* t, gv_vec* const* p) {
    NEED(c, C >= 0, "gv_screen_dev: the number of columns is negative");
    if (C == 0) return 0;
    NEED(c, u && r, "gv_screen_dev: the arrays of column handles are NULL");
    const bool dosage = screen_dosage(c);      // gv_set_screen_dosage is on and dosage codes are resident
    NEED(c, dosage || !c->dense.resident, "gv_screen_dev: no screen is defined for methylation or dosage data (2-bit genotypes only)");
    NEED(c, c->have_stats && c->mask2 && (dosage ? c->dense.qss != nullptr : c->counts != nullptr),
         "ATx: bed and marker statistics must be set first");
    NEED(c, c->alpha_scale == 1.0, "gv_screen_dev: the marker statistics must be those of alpha_scale = 1 (r is a correlation)");
    NEED(c, c->nonas >= 3, "gv_screen_dev: fewer than 3 individuals with a phenotype leave the test no degree of freedom");
    std::vector<const double*> us;
    std::vector<double*> rs;
    if (batch_args(c, "gv_screen_dev", C, u, r, "u", GV_SPACE_N, us, rs)) return 1;
    // t and p: M-space vectors of this context, distinct from each other, from r and from the inputs
    std::unordered_set<const gv_vec*> seen;
    for (int64_t j = 0; j < C; j++) { seen.insert(u[j]); seen.insert(r[j]); }
    for (gv_vec* const* arr : {t, p}) {
        if (!arr) continue;
        const char* an = arr == t ? "t" : "p";
        for (int64_t j = 0; j < C; j++) {
            if (!arr[j]) return fail(c, "gv_screen_dev: the handle of column %lld is NULL", (long long)j);
            const std::string w = "gv_screen_dev: column " + std::to_string((long long)j);
            if (!vec_ok(c, arr[j], GV_SPACE_M)) return vec_need(c, w.c_str(), an, arr[j], GV_SPACE_M);
            if (!seen.insert(arr[j]).second) return fail(c, "gv_screen_dev: column %lld: two outputs are the same vector", (long long)j);
        }
    }
    if (atxm_device(c, C, us.data(), rs.data())) return 1;
    if (c->M == 0) return 0;
    const double rfac = sqrt((double)c->N) / (double)(c->nonas - 1), nu = (double)(c->nonas - 2);
    for (int64_t j0 = 0; j0 < C; j0 += gvx::CP_MAX) {
        const int nc = (int)(C - j0 < gvx::CP_MAX ? C - j0 : gvx::CP_MAX);
        ScreenCols sc{};
        for (int j = 0; j < nc; j++) {
            sc.r[j] = rs[(size_t)(j0 + j)];
            sc.t[j] = t ? t[j0 + j]->d : nullptr;
            sc.p[j] = p ? p[j0 + j]->d : nullptr;
        }
        hipLaunchKernelGGL(k_screen_fin, dim3(nblk(c->M, 256), nc), dim3(256), 0, c->stream, sc, c->M, c->counts, c->mave, c->msig,
                           dosage ? c->dense.qss : nullptr, rfac, nu);
    }
    KCHK(c);
    return 0;
}

}  // extern "C"
