// gv_dense_mfma.hip -- fixed-point i8 MFMA route for the products of 8-bit dosage codes (gv_set_dosage_route(ctx, 1); DESIGN.md
// section 14, "Fixed-point route").  Opt-in: the default route stays the k_dosage_* kernels of gv_dense.hip.
//
// The arithmetic is that of gv_mfma.hip (its header): a vector enters a product as q = rint(v 2^(54-e)), 2^(e-1) <= max|v| < 2^e, one
// exponent per vector, in 7 balanced base-256 digits in [-128, 127]; the products of digits and codes are exact int32 sums of
// v_mfma_i32_16x16x64_i8, the digit planes are recombined in exact int64 limbs and rounded once.  A u8 code b becomes the i8 operand
// byte b - 128 by one xor 0x80808080 per dword; the 128 is taken back in exact integers (below).
//
// Data: the resident pitched marker-major rows (DenseData::rows) as they are -- no second copy.  NA = false only: every code is a value.
//
// Digits (k_dm_quant): one buffer of 16 columns per K-entry, columns 0..6 the digits of vector slot a, 8..14 those of slot b, 7 and 15
// zero; a one-vector pass leaves the columns of slot b zero and costs the same MFMAs.  Order: K-block kb = k >> 6 is 1 KiB, inside it
// lane (c, g) of the B operand -- byte ((g * 16 + c) * 16 + j) -- holds digit column c of K-entry 64 kb + 16 g + j.  The A operand of the
// same MFMA holds, in lane (r, g), the 16 codes of tile row r at the K-entries 64 kb + 16 g + j: both operands agree byte for byte.
// Entries from K up to the padded length carry zero digits: the codes there (row padding: zeros in memory, -128 after the bias; rows
// re-read past the last marker) multiply zeros.
//
//   ATx (K = individuals): a wave owns 8 tiles of 16 marker rows and walks the individuals in steps of 128: per tile two 16-byte loads
//       per lane, (r, g) taking bytes [16 g, 16 g + 16) of row r at k0 and at k0 + 64 -- back to back, so the two halves of a row's
//       128-byte line are consumed together -- and no cross-lane movement.  Per marker S1 = sum_n (b - 128) q_n comes from the MFMAs and
//       Q = sum_n q_n, an exact integer, from the limb sums of the quantisation:
//           out[m] = msig[m] scale_x (S1[m] - (mu'[m] - 128) Q) 2^(e-54) / sqrt(N),   then tau out + gam2 addx.
//   Ax (K = markers): c_m = msig_m scale_x x_m in digits, e_m = (mu'_m - 128) c_m quantised on the grid 2^7 coarser (|e| <= 128 |c|, so
//       |qe| < 2^54 too): out[n] = (T[n] - 128 E) 2^(ec-54) post with T[n] = sum_m (b_mn - 128) qc_m from the MFMAs and E = sum_m qe_m one
//       exact integer per pass -- the subtraction happens in integers, before the one rounding.  The matrix is marker-major, the operand
//       needs 16 markers of ONE individual in a lane's 16 bytes: a lane loads 8 bytes (8 individuals) from each of 16 rows and transposes
//       4 x 4 byte blocks in registers (v_perm_b32, 0.5 instructions per entry); tile s of a wave is the individuals n0 + 8 r + s.
//       No phenotype mask (as the dense Ax); pad slots of the output are exact zeros.
//
// The int32 invariant: see gvdm::SEG_MAX (gv_internal.h) and seg_steps() below, the one place that cuts K-segments.  Every sum is an
// integer: the results depend on no segment length, no order and no grid (bit-reproducible); there are no atomics.
#include "gv_internal.h"
#include "gv_dense_atxm_plan.h"
#include "gv_dense_fx.h"

namespace {

using gvdm::limb_total; using gvdm::limbs_to_double; using gvdm::gather; using gvdm::atx_value;

constexpr int WAVE = 64;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int NB = gvdm::BLOCKS;            // most blocks of a max / quantisation launch (their partials are summed by every consumer)
constexpr uint32_t BIAS = 0x80808080u;      // u8 code b -> i8 operand byte b - 128

__device__ inline double wave_max(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
    return v;
}
__device__ inline long long wave_sum_ll(long long v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// What is quantised: ax == 0: v itself (the ATx operand p); ax == 1: c = msig scale_x x (the weight route 0 forms), and beside it
// e = (mu' - 128) c for the limb sums.
struct Operand { const double* v[2]; const double* msig; const double* mu; double wscale; int ax; };
__device__ inline double operand(const Operand& o, int slot, int64_t i) {
    const double x = o.v[slot][i];
    return o.ax ? o.msig[i] * o.wscale * x : x;
}

// ---- max |v| per slot: block partials (a NaN or an infinity raises the partial to +inf, as k_prep_atx does)
__global__ __launch_bounds__(256) void k_dm_max(Operand o, int64_t n, double* __restrict__ pmax) {
    __shared__ double sh[4];
    const int slot = blockIdx.y;
    double mx = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = operand(o, slot, i);
        mx = isfinite(v) ? fmax(mx, fabs(v)) : __longlong_as_double(0x7ff0000000000000LL);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) pmax[slot * NB + blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// ---- digits.  Every block adds the block maxima up for itself by a fixed tree (same order: same bits), block 0 stores the slot's
// scal = 2^(e-54) (0 for a zero vector, NaN when an entry is not finite: every output of the product is NaN then, as in kernel mode 1).
// A thread quantises 4 consecutive K-entries: one dword per digit column.  limb[(slot NB + block) 2 + {0, 1}] = the block's sums of
// the high (q >> 32, signed) and low (q & 0xffffffff) limbs of q (ATx) or of qe (Ax); slot b of a one-vector pass (v[1] == NULL) gets
// zero digits.  kpad: K rounded up to 128; entries K <= k < kpad get zero digits.
__global__ __launch_bounds__(256) void k_dm_quant(Operand o, int64_t n, int64_t kpad, const double* __restrict__ pmax, int nbmax,
                                                  uint32_t* __restrict__ dig, long long* __restrict__ limb, double* __restrict__ scal) {
    __shared__ double shm[256];
    __shared__ long long shl[2][4];
    const int slot = blockIdx.y;
    const bool absent = o.v[slot] == nullptr;
    double mx = 0.0;
    if (!absent)
        for (int b = threadIdx.x; b < nbmax; b += 256) mx = fmax(mx, pmax[slot * NB + b]);
    shm[threadIdx.x] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) shm[threadIdx.x] = fmax(shm[threadIdx.x], shm[threadIdx.x + off]);
        __syncthreads();
    }
    const double amax = shm[0];
    double mult = 0.0, inv = 0.0;
    if (amax > 0.0 && amax <= 1.7976931348623157e308) {
        int sh = 54 - (ilogb(amax) + 1);
        if (sh > 1000) sh = 1000;      // (a vector below 2^-946 keeps a representable multiplier: fewer bits, the same formulas)
        mult = ldexp(1.0, sh);
        inv = ldexp(1.0, -sh);
    } else if (amax != 0.0)
        inv = __longlong_as_double(0x7ff8000000000000LL);
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[slot] = inv;
    const double mult_e = mult * 0x1p-7;
    long long hi = 0, lo = 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < kpad / 4; t += (int64_t)gridDim.x * 256) {
        const int64_t k = 4 * t;
        uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (absent || k + i >= n) continue;
            const double val = operand(o, slot, k + i);
            long long q = (long long)rint(val * mult);
            const long long ql = o.ax ? (long long)rint((o.mu[k + i] - 128.0) * val * mult_e) : q;
            hi += ql >> 32;
            lo += ql & 0xFFFFFFFFLL;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const long long dg = (long long)(signed char)(q & 0xFF);      // balanced digit in [-128, 127]
                q = (q - dg) >> 8;
                d[c] |= (uint32_t)(dg & 0xFF) << (8 * i);
            }
        }
        uint32_t* w = dig + (k >> 6) * 256 + ((k >> 4) & 3) * 64 + slot * 32 + ((k & 15) >> 2);
#pragma unroll
        for (int c = 0; c < 8; c++) w[c * 4] = d[c];
    }
    hi = wave_sum_ll(hi);
    lo = wave_sum_ll(lo);
    if ((threadIdx.x & (WAVE - 1)) == 0) { shl[0][threadIdx.x >> 6] = hi; shl[1][threadIdx.x >> 6] = lo; }
    __syncthreads();
    if (threadIdx.x < 2)
        limb[((int64_t)slot * NB + blockIdx.x) * 2 + threadIdx.x] =
            (shl[threadIdx.x][0] + shl[threadIdx.x][1]) + (shl[threadIdx.x][2] + shl[threadIdx.x][3]);
}

// ---- ATx streaming kernel.  partial[(seg rows_p + row) 16 + column] (int32), rows_p = 128 row blocks.
constexpr int ATX_T = 8;      // tiles of 16 rows per wave
__global__ __launch_bounds__(256) void k_dm_atx(const uint8_t* __restrict__ A, int64_t M, int64_t pitch, int64_t steps, int64_t seg_steps,
                                                int64_t nrb, uint32_t nbx, const u32x4* __restrict__ dig, int32_t* __restrict__ part,
                                                int64_t rows_p) {
    const int lane = threadIdx.x & (WAVE - 1), r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t seg = blockIdx.x / nbx, rb = (int64_t)(blockIdx.x % nbx) * 4 + wave;
    if (rb >= nrb) return;
    const uint8_t* row[ATX_T];
#pragma unroll
    for (int i = 0; i < ATX_T; i++) {
        int64_t m = rb * 128 + 16 * i + r;
        if (m >= M) m = M - 1;      // (a row block's tail re-reads the last row; its sums are never read)
        row[i] = A + m * pitch + 16 * g;
    }
    v4i acc[ATX_T];
#pragma unroll
    for (int i = 0; i < ATX_T; i++) acc[i] = (v4i){0, 0, 0, 0};
    const int64_t s0 = seg * seg_steps, s1 = s0 + seg_steps < steps ? s0 + seg_steps : steps;
    for (int64_t st = s0; st < s1; st++) {
        const int64_t k0 = st * 128;
        // the row pitch is a multiple of 64, not of 128: the second half of the last step may lie past the row -- the first half is read
        // again instead (its digits are zeros: k0 + 64 >= pitch >= N)
        const int64_t k1 = k0 + 64 < pitch ? k0 + 64 : k0;
        u32x4 a[ATX_T][2];
#pragma unroll
        for (int i = 0; i < ATX_T; i++) {
            a[i][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row[i] + k0));
            a[i][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row[i] + k1));
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u32x4 bq = dig[(2 * st + h) * 64 + lane];
            const v4i B = {(int)bq.x, (int)bq.y, (int)bq.z, (int)bq.w};
#pragma unroll
            for (int i = 0; i < ATX_T; i++) {
                const u32x4 x = a[i][h] ^ BIAS;
                const v4i X = {(int)x.x, (int)x.y, (int)x.z, (int)x.w};
                acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(X, B, acc[i], 0, 0, 0);
            }
        }
    }
    // C layout: lane (c, g), register reg = row 4 g + reg of the tile, column c
#pragma unroll
    for (int i = 0; i < ATX_T; i++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int64_t rw = rb * 128 + 16 * i + 4 * g + reg;
            part[(seg * rows_p + rw) * 16 + r] = acc[i][reg];
        }
}

// ATx epilogue: blockIdx.y = slot
struct FinAtx { double* out[2]; const double* addx[2]; };
__global__ __launch_bounds__(256) void k_dm_fin_atx(const int32_t* __restrict__ part, int segs, int64_t rows_p, int64_t M,
                                                    const long long* __restrict__ limb, int nbq, const double* __restrict__ scal,
                                                    const double* __restrict__ dmu, const double* __restrict__ msig, double wscale,
                                                    double scale, FinAtx a, double tau, double gam2) {
    const int v = blockIdx.y;
    long long qh, ql;
    limb_total(limb + (int64_t)v * NB * 2, nbq, qh, ql);
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long long sh, sl;
    gather(part, segs, rows_p, m, 16, 8 * v, sh, sl);
    const double res = atx_value(dmu[m], msig[m], wscale, scale, scal[v], qh, ql, sh, sl);
    a.out[v][m] = a.addx[v] ? fma(tau, res, gam2 * a.addx[v][m]) : res;
}

// ---- Ax streaming kernel.  A wave owns 128 individuals (column block cb) and a segment of marker steps (64 markers each).
__device__ inline void transpose4x4_bytes(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&o)[4]) {
    const uint32_t a0 = __builtin_amdgcn_perm(w1, w0, 0x05010400u), a1 = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
    const uint32_t b0 = __builtin_amdgcn_perm(w3, w2, 0x05010400u), b1 = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
}
__global__ __launch_bounds__(256) void k_dm_ax(const uint8_t* __restrict__ A, int64_t M, int64_t pitch, int64_t steps, int64_t seg_steps,
                                               int64_t ncb, uint32_t nbx, const u32x4* __restrict__ dig, int32_t* __restrict__ part,
                                               int64_t rows_p) {
    const int lane = threadIdx.x & (WAVE - 1), r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t seg = blockIdx.x / nbx, cb = (int64_t)(blockIdx.x % nbx) * 4 + wave;
    if (cb >= ncb) return;
    // 8 individuals per lane; past the pitch (a multiple of 64: a piece is inside or outside as a whole) the block's first piece is read
    // again -- those individuals are pad slots, their sums are never read.  The lane's offset fits 32 bits: pitch <= gvdm::PITCH_MAX.
    int64_t col = cb * 128 + 8 * r;
    if (col >= pitch) col = cb * 128;
    const uint32_t lane_off = (uint32_t)(16 * g * pitch + col);
    v4i acc[8];
#pragma unroll
    for (int s = 0; s < 8; s++) acc[s] = (v4i){0, 0, 0, 0};
    const int64_t s0 = seg * seg_steps, s1 = s0 + seg_steps < steps ? s0 + seg_steps : steps;
    for (int64_t st = s0; st < s1; st++) {
        const int64_t k0 = st * 64;
        u32x2 x[16];
        if (k0 + 64 <= M) {
            const uint8_t* base = A + k0 * pitch;
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(base + j * pitch + lane_off));
        } else {      // the last step: rows past the last marker re-read it (their digits are zeros)
#pragma unroll
            for (int j = 0; j < 16; j++) {
                int64_t m = k0 + 16 * g + j;
                if (m >= M) m = M - 1;
                x[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(A + m * pitch + col));
            }
        }
        const u32x4 bq = dig[st * 64 + lane];
        const v4i B = {(int)bq.x, (int)bq.y, (int)bq.z, (int)bq.w};
        // A operand of tile s (individual n0 + 8 r + s): dword w, byte t = marker 16 g + 4 w + t
        uint32_t t[8][4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t o[4];
            transpose4x4_bytes(x[4 * w].x ^ BIAS, x[4 * w + 1].x ^ BIAS, x[4 * w + 2].x ^ BIAS, x[4 * w + 3].x ^ BIAS, o);
#pragma unroll
            for (int s = 0; s < 4; s++) t[s][w] = o[s];
            transpose4x4_bytes(x[4 * w].y ^ BIAS, x[4 * w + 1].y ^ BIAS, x[4 * w + 2].y ^ BIAS, x[4 * w + 3].y ^ BIAS, o);
#pragma unroll
            for (int s = 0; s < 4; s++) t[4 + s][w] = o[s];
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const v4i X = {(int)t[s][0], (int)t[s][1], (int)t[s][2], (int)t[s][3]};
            acc[s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(X, B, acc[s], 0, 0, 0);
        }
    }
#pragma unroll
    for (int s = 0; s < 8; s++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int64_t n = cb * 128 + 8 * (4 * g + reg) + s;
            part[(seg * rows_p + n) * 16 + r] = acc[s][reg];
        }
}

// Ax epilogue: out[n] = (T[n] - 128 E) scal post for n < N, exact zeros at the pad slots; blockIdx.y = slot
__global__ __launch_bounds__(256) void k_dm_fin_ax(const int32_t* __restrict__ part, int segs, int64_t rows_p, int64_t N, int64_t npad,
                                                   const long long* __restrict__ limb, int nbq, const double* __restrict__ scal,
                                                   double post, double* __restrict__ outa, double* __restrict__ outb) {
    const int v = blockIdx.y;
    long long eh, el;
    limb_total(limb + (int64_t)v * NB * 2, nbq, eh, el);
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    double val = 0.0;
    if (n < N) {
        long long th, tl;
        gather(part, segs, rows_p, n, 16, 8 * v, th, tl);
        val = limbs_to_double(th - 128 * eh, tl - 128 * el) * scal[v] * post;
    }
    (v == 0 ? outa : outb)[n] = val;
}

inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }
inline int64_t round128(int64_t k) { return (k + 127) / 128 * 128; }

// THE place that cuts K-segments.  No int32 accumulation of a streaming kernel may span more than gvdm::SEG_MAX K-entries (a K-entry
// adds at most 128 * 128 to a column sum): a segment is at most `cap` <= SEG_MAX entries (GV_DOSAGE_MFMA_SEG), rounded DOWN to whole
// K-steps of the kernel, at least one.  `want` segments are asked for to fill the device; the bound may only raise their number.
static_assert(gvdm::SEG_MAX * 128 * 128 <= 2147483647LL, "an int32 column sum over SEG_MAX K-entries must fit");
gvdm::Shape cut(int64_t K, int kstep, int64_t blocks, int64_t cap, int cus) {
    const gvdx::Cut ct = gvdx::cut_segments(K, kstep, blocks, cap, cus, gvdm::SEG_MAX);      // (gv_dense_atxm_plan.h: the arithmetic)
    gvdm::Shape sh;
    sh.blocks = blocks;
    sh.steps = ct.steps;
    sh.seg_steps = ct.seg_steps;
    sh.segs = ct.segs;
    return sh;
}

void quantise(hipStream_t s, const Operand& o, int nv, int64_t n, const gvdm::Scratch& w) {
    const int64_t kpad = round128(n);
    const int64_t b1 = (n + 255) / 256, b2 = (kpad / 4 + 255) / 256;
    const int nbm = (int)(b1 < 1 ? 1 : (b1 > NB ? NB : b1)), nbq = (int)(b2 < 1 ? 1 : (b2 > NB ? NB : b2));
    hipLaunchKernelGGL(k_dm_max, dim3(nbm, nv), dim3(256), 0, s, o, n, w.pmax);
    hipLaunchKernelGGL(k_dm_quant, dim3(nbq, 2), dim3(256), 0, s, o, n, kpad, w.pmax, nbm, (uint32_t*)w.dig, w.limb, w.scal);
}
int quant_blocks(int64_t n) {
    const int64_t b2 = (round128(n) / 4 + 255) / 256;
    return (int)(b2 < 1 ? 1 : (b2 > NB ? NB : b2));
}

}  // namespace

namespace gvdm {

static_assert(gvdx::SEG_MAX == SEG_MAX && gvdx::ATX_KSTEP == ATX_KSTEP && gvdx::QUANT_BLOCKS == BLOCKS, "the plan header's constants");

void quantise_atx(hipStream_t s, const double* pa, const double* pb, int64_t n, const Scratch& w) {
    const Operand o = {{pa, pb}, nullptr, nullptr, 1.0, 0};
    quantise(s, o, pb ? 2 : 1, n, w);
}
int quant_blocks_of(int64_t n) { return quant_blocks(n); }

Shape atx_shape(int64_t N, int64_t M, int cus, int64_t cap) { return cut(N, ATX_KSTEP, (M + 127) / 128, cap, cus); }
Shape ax_shape(int64_t N, int64_t M, int cus, int64_t cap) { return cut(M, AX_KSTEP, (gvd::row_pitch(N) + 127) / 128, cap, cus); }

hipError_t reserve(Scratch& w, int64_t N, int64_t M, int cus, int64_t cap) {
    const Shape sa = atx_shape(N, M, cus, cap), sx = ax_shape(N, M, cus, cap);
    const size_t dig = (size_t)round128(N > M ? N : M) * 16;
    const size_t pa = (size_t)sa.segs * (size_t)sa.blocks * 128 * 16, px = (size_t)sx.segs * (size_t)sx.blocks * 128 * 16;
    const size_t part = pa > px ? pa : px;
    hipError_t e;
    if (dig > w.dig_cap) {
        if (w.dig) (void)hipFree(w.dig);
        w.dig = nullptr;
        w.dig_cap = 0;
        if ((e = hipMalloc(&w.dig, dig)) != hipSuccess) return e;
        w.dig_cap = dig;
    }
    if (part > w.part_cap) {
        if (w.part) (void)hipFree(w.part);
        w.part = nullptr;
        w.part_cap = 0;
        if ((e = hipMalloc(&w.part, sizeof(int32_t) * part)) != hipSuccess) return e;
        w.part_cap = part;
    }
    if (!w.pmax) {      // one allocation: 2 NB block maxima | 4 NB limb sums | 2 scalars
        if ((e = hipMalloc(&w.pmax, sizeof(double) * (2 * BLOCKS + 4 * BLOCKS + 2))) != hipSuccess) return e;
        w.limb = reinterpret_cast<long long*>(w.pmax + 2 * BLOCKS);
        w.scal = w.pmax + 6 * BLOCKS;
    }
    return hipSuccess;
}
void release(Scratch& w) {
    for (void** q : {&w.dig, (void**)&w.part, (void**)&w.pmax})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    w = Scratch();
}

void atx(hipStream_t s, int nv, const gvd::View& v, const Scratch& w, const Shape& sh, const double* pa, const double* pb, double scale,
         double* outa, double* outb, const double* addxa, const double* addxb, double tau, double gam2, hipEvent_t ev0, hipEvent_t ev1) {
    if (v.M <= 0) return;
    const Operand o = {{pa, nv == 2 ? pb : nullptr}, nullptr, nullptr, 1.0, 0};
    quantise(s, o, nv, v.N, w);
    const int64_t rows_p = sh.blocks * 128;
    const uint32_t nbx = (uint32_t)((sh.blocks + 3) / 4);
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_dm_atx, dim3(nbx * (uint32_t)sh.segs), dim3(256), 0, s, (const uint8_t*)v.rows, v.M, v.pitch, sh.steps, sh.seg_steps,
                       sh.blocks, nbx, (const u32x4*)w.dig, w.part, rows_p);
    if (ev1) (void)hipEventRecord(ev1, s);
    const FinAtx f = {{outa, outb}, {addxa, addxb}};
    hipLaunchKernelGGL(k_dm_fin_atx, dim3(nblk(v.M, 256), nv), dim3(256), 0, s, w.part, sh.segs, rows_p, v.M, w.limb, quant_blocks(v.N),
                       w.scal, v.centre, v.msig, v.wscale, scale, f, tau, gam2);
}

void ax(hipStream_t s, int nv, const gvd::View& v, const Scratch& w, const Shape& sh, const double* xa, const double* xb, int64_t npad,
        double post, double* outa, double* outb, hipEvent_t ev0, hipEvent_t ev1) {
    if (v.M <= 0) return;
    const Operand o = {{xa, nv == 2 ? xb : nullptr}, v.msig, v.centre, v.wscale, 1};
    quantise(s, o, nv, v.M, w);
    const int64_t rows_p = sh.blocks * 128;
    const uint32_t nbx = (uint32_t)((sh.blocks + 3) / 4);
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_dm_ax, dim3(nbx * (uint32_t)sh.segs), dim3(256), 0, s, (const uint8_t*)v.rows, v.M, v.pitch, sh.steps, sh.seg_steps,
                       sh.blocks, nbx, (const u32x4*)w.dig, w.part, rows_p);
    if (ev1) (void)hipEventRecord(ev1, s);
    hipLaunchKernelGGL(k_dm_fin_ax, dim3(nblk(npad, 256), nv), dim3(256), 0, s, w.part, sh.segs, rows_p, v.N, npad, w.limb,
                       quant_blocks(v.M), w.scal, post, outa, outb);
}

}  // namespace gvdm
