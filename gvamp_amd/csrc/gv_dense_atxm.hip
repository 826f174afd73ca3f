// gv_dense_atxm.hip -- R = A^T Y for CP in {4, 8} phenotype columns per pass over resident 8-bit dosage codes on the fixed-point i8 MFMA
// route (gv_atxm_dev under gv_set_dosage_route(ctx, 1)).  k_dm_atx of gv_dense_mfma.hip generalised: the same
// resident pitched rows, no second copy, no atomics, every sum an exact integer -- column j is bit-identical to gv_atx_dev of it alone.
//
// Digits: the quantisation of gv_dense_mfma.hip (k_dm_max / k_dm_quant through gvdm::quantise_atx), one launch per column PAIR into the
// pair's own B-operand buffer of 1 KiB per 64 K-entries in the existing 16-column order (slot a in columns 0..6, slot b in 8..14, 7 and
// 15 zero), with the pair's own block maxima, limb sums Q = sum q and scalars.  A pair with one column leaves slot b zero, a pair
// without a column (the tail of a last pass) is a buffer of zeros.  K-entries N <= k < round128(N) carry zero digits: they mask the row
// padding and the half-step read again at the end of a row.
//
// Streaming loop: a wave owns T tiles of 16 marker rows and walks the individuals in steps of 128; per tile the two 16-byte loads per
// lane of k_dm_atx and the xor 0x80808080 happen ONCE, then CP / 2 MFMAs per half-step run against the CP / 2 digit blocks, which every
// wave fetches from global memory (L2) as k_dm_atx does.  Accumulators: T * CP / 2 * 4 registers per lane.  T per CP: AtxmTiles below.
//
// Edges (each as in k_dm_atx): the row clamp m >= M -> M - 1; k1 = k0 when k0 + 64 >= pitch; idle waves of the last workgroup return;
// the partials hold whole 128-row blocks x segments x CP * 8 int32 columns; a digit read is at most K-entry round128(N) - 1.
// Segments: the cut of the one-vector product (gvdm::atx_shape), so the int32 invariant of gvdm::SEG_MAX holds unchanged -- a column's
// accumulator sees what k_dm_atx's sees.  The epilogue adds the int32 partials in int64 and rounds by gvdm::atx_value, the function
// k_dm_fin_atx calls.
#include "gv_internal.h"
#include "gv_dense_fx.h"

namespace {

constexpr int WAVE = 64;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int NB = gvdm::BLOCKS;
constexpr uint32_t BIAS = 0x80808080u;      // u8 code b -> i8 operand byte b - 128
constexpr int CP_MAX = 8;

// tiles of 16 rows per wave: the library's pick per CP.  No instantiation spills (the resource report), so the
// measurement decides: at 20 000 x 800 000 a pass of the CP = 4 instantiation takes 4.53 ms with 4 tiles and 4.94 ms with 8, a pass of the
// CP = 8 instantiation 5.24 ms with 4 tiles and 4.99 ms with 8.  GV_ATXM_TILES (development) runs the other instantiation
template <int CP> struct AtxmTiles;
template <> struct AtxmTiles<4> { static constexpr int T = 4; };
template <> struct AtxmTiles<8> { static constexpr int T = 8; };

// partial[((seg rows_p + row) CP / 2 + pair) 16 + column] (int32), rows_p = 128 row blocks; nrb = waves with rows: ceil(M / (16 T))
template <int CP, int T>
__global__ __launch_bounds__(256) void k_dm_atxm(const uint8_t* __restrict__ A, int64_t M, int64_t pitch, int64_t steps, int64_t seg_steps,
                                                 int64_t nrb, uint32_t nbx, const u32x4* __restrict__ dig, int64_t dig_stride,
                                                 int32_t* __restrict__ part, int64_t rows_p) {
    constexpr int NP = CP / 2;
    const int lane = threadIdx.x & (WAVE - 1), r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t seg = blockIdx.x / nbx, rb = (int64_t)(blockIdx.x % nbx) * 4 + wave;
    if (rb >= nrb) return;
    const uint8_t* row[T];
#pragma unroll
    for (int i = 0; i < T; i++) {
        int64_t m = rb * (16 * T) + 16 * i + r;
        if (m >= M) m = M - 1;      // (a row block's tail re-reads the last row; its sums are never read)
        row[i] = A + m * pitch + 16 * g;
    }
    v4i acc[T][NP];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int p = 0; p < NP; p++) acc[i][p] = (v4i){0, 0, 0, 0};
    const int64_t s0 = seg * seg_steps, s1 = s0 + seg_steps < steps ? s0 + seg_steps : steps;
    for (int64_t st = s0; st < s1; st++) {
        const int64_t k0 = st * 128;
        // the row pitch is a multiple of 64, not of 128: the second half of the last step may lie past the row -- the first half is read
        // again instead (its digits are zeros: k0 + 64 >= pitch >= N)
        const int64_t k1 = k0 + 64 < pitch ? k0 + 64 : k0;
        u32x4 a[T][2];
#pragma unroll
        for (int i = 0; i < T; i++) {
            a[i][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row[i] + k0));
            a[i][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row[i] + k1));
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            v4i B[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const u32x4 bq = dig[p * dig_stride + (2 * st + h) * 64 + lane];      // (2 st + h) 64 + lane < 128 steps = round128(N)
                B[p] = (v4i){(int)bq.x, (int)bq.y, (int)bq.z, (int)bq.w};
            }
#pragma unroll
            for (int i = 0; i < T; i++) {
                const u32x4 x = a[i][h] ^ BIAS;
                const v4i X = {(int)x.x, (int)x.y, (int)x.z, (int)x.w};
#pragma unroll
                for (int p = 0; p < NP; p++) acc[i][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(X, B[p], acc[i][p], 0, 0, 0);
            }
        }
    }
    // C layout: lane (c, g), register reg = row 4 g + reg of the tile, column c of the pair
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int64_t rw = rb * (16 * T) + 16 * i + 4 * g + reg;      // < nrb 16 T <= rows_p (16 T divides 128)
#pragma unroll
            for (int p = 0; p < NP; p++) part[((seg * rows_p + rw) * NP + p) * 16 + r] = acc[i][p][reg];
        }
}

// epilogue of column blockIdx.y (k_dm_fin_atx without addx): pair = column >> 1, slot = column & 1; small = the pairs' blocks of
// 2 NB maxima | 4 NB limb sums | 2 scalars, small_stride doubles apart
struct OutCols { double* out[CP_MAX]; };
__global__ __launch_bounds__(256) void k_dm_fin_atxm(const int32_t* __restrict__ part, int segs, int64_t rows_p, int64_t M, int cp,
                                                     const double* __restrict__ small, int64_t small_stride, int nbq,
                                                     const double* __restrict__ dmu, const double* __restrict__ msig, double wscale,
                                                     double scale, OutCols a) {
    const int v = blockIdx.y, slot = v & 1;
    const double* sm = small + (int64_t)(v >> 1) * small_stride;
    const long long* limb = reinterpret_cast<const long long*>(sm + 2 * NB) + (int64_t)slot * NB * 2;
    const double scal = sm[6 * NB + slot];
    long long qh, ql;
    gvdm::limb_total(limb, nbq, qh, ql);
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long long sh, sl;
    gvdm::gather(part, segs, rows_p, m, cp * 8, 8 * v, sh, sl);
    a.out[v][m] = gvdm::atx_value(dmu[m], msig[m], wscale, scale, scal, qh, ql, sh, sl);
}

template <int CP, int T>
void launch_pass(hipStream_t s, const gvd::View& v, const gvdm::Shape& sh, const u32x4* dig, int64_t dig_stride, int32_t* part) {
    const int64_t nrb = (v.M + 16 * T - 1) / (16 * T);
    const uint32_t nbx = (uint32_t)((nrb + 3) / 4);
    hipLaunchKernelGGL((k_dm_atxm<CP, T>), dim3(nbx * (uint32_t)sh.segs), dim3(256), 0, s, (const uint8_t*)v.rows, v.M, v.pitch, sh.steps,
                       sh.seg_steps, nrb, nbx, dig, dig_stride, part, sh.blocks * 128);
}

}  // namespace

namespace gvdm {

int atxm_tiles(int cp) { return cp == 4 ? AtxmTiles<4>::T : AtxmTiles<8>::T; }

hipError_t atxm_pass(hipStream_t s, const gvd::View& v, const Shape& sh, int cp, int tiles, int ncols, const double* const* p, double* const* out,
                     double scale, char* dig, size_t pair_dig_bytes, int32_t* part, char* small, size_t pair_small_bytes) {
    if (v.M <= 0 || ncols <= 0) return hipSuccess;
    for (int pr = 0; pr < cp / 2; pr++) {
        char* pd = dig + (size_t)pr * pair_dig_bytes;
        if (2 * pr >= ncols) {      // a pair without a column: zero digits
            const hipError_t e = hipMemsetAsync(pd, 0, pair_dig_bytes, s);
            if (e != hipSuccess) return e;
            continue;
        }
        Scratch w;
        w.dig = pd;
        w.pmax = reinterpret_cast<double*>(small + (size_t)pr * pair_small_bytes);
        w.limb = reinterpret_cast<long long*>(w.pmax + 2 * BLOCKS);
        w.scal = w.pmax + 6 * BLOCKS;
        quantise_atx(s, p[2 * pr], 2 * pr + 1 < ncols ? p[2 * pr + 1] : nullptr, v.N, w);
    }
    const int64_t dig_stride = (int64_t)(pair_dig_bytes / 16);
    if (!tiles) tiles = atxm_tiles(cp);
    if (cp == 4 && tiles == 4) launch_pass<4, 4>(s, v, sh, (const u32x4*)dig, dig_stride, part);
    else if (cp == 4) launch_pass<4, 8>(s, v, sh, (const u32x4*)dig, dig_stride, part);
    else if (tiles == 4) launch_pass<8, 4>(s, v, sh, (const u32x4*)dig, dig_stride, part);
    else launch_pass<8, 8>(s, v, sh, (const u32x4*)dig, dig_stride, part);
    OutCols oc{};
    for (int j = 0; j < ncols; j++) oc.out[j] = out[j];
    hipLaunchKernelGGL(k_dm_fin_atxm, dim3((unsigned)((v.M + 255) / 256), ncols), dim3(256), 0, s, part, sh.segs, sh.blocks * 128, v.M, cp,
                       (const double*)small, (int64_t)(pair_small_bytes / 8), quant_blocks_of(v.N), v.centre, v.msig, v.wscale, scale, oc);
    return hipSuccess;
}

}  // namespace gvdm
