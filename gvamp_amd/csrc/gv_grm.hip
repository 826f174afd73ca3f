// gv_grm.hip -- the standardised genetic relationship matrix of the resident 2-bit genotypes (gv_grm_weights, gv_grm_block, gv_grm_pairs;
// DESIGN.md section 28): A = Z Z^T / M_ij with real per-marker weights, the second N x N product of the tree beside gv_king.hip and the
// first user of the fp64 matrix pipe (v_mfma_f64_16x16x4_f64).
//
// With a in {0, 1, 2} the allele count the tile layout stores as r' = a (r' = 3: missing):
//   k_grm_freq   one workgroup per 64-marker row group: n_m = #present and s_m = sum a over the N individuals in exact integers, then the
//                weights of the contract (mu, rs), the four values an entry of the marker can take, z[c] = ((double)c - mu) rs for
//                c = 0, 1, 2 and 0 for c = 3, and the selector mask of the count plane (KING's: byte t of quad q = 4 where marker
//                4 q + t does not count).  A marker that does not count has z[.] = 0: it adds nothing to S.
//   k_grm_block  one workgroup of 256 threads per pair of 64-individual groups (I <= J); the K loop runs over the shard's 64-marker row
//                groups.  Per row group the workgroup stages the 1 KiB of 2-bit codes of either side, the 64 x 4 values z[c] and the 16
//                selector masks in LDS (4.1 KiB, two buffers: one barrier per row group); every lane then builds its own operands in
//                registers -- one 2-bit extract and one 8-byte LDS look-up per fp64 operand.  Each of the 4 waves owns a 32 x 32
//                quarter: 4 tiles of v_mfma_f64_16x16x4_f64 for S (16 K-steps of 4 markers per row group) and 4 tiles of ONE
//                v_mfma_i32_16x16x64_i8 on the present-and-counting plane for M_ij.  The rows of the i8 A operand are permuted so that
//                both results of a pair land in the same lane and register: the f64 C/D map is row = (lane >> 4) + 4 reg, the i32 one
//                row = 4 (lane >> 4) + reg.
// S is one fp64 accumulator per pair, summed in ascending K-step by the matrix pipe: its order is a function of (M, use) alone, never of
// the launch, the rectangle or the list.  (i, j) and (j, i) are the same products in the same order.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "gv_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v4d __attribute__((ext_vector_type(4)));

// M_ij is an int32 sum of at most 1 per marker: M <= 2^31 - 1, as KING
constexpr int64_t GRM_M_MAX = 2147483647LL;
constexpr int64_t GRM_BLOCKS_MAX = 2147483647LL;       // workgroups of one launch (a 1-D grid)

// the count plane as a byte look-up (gv_king.hip): v_perm_b32 with the selector byte c = r' (| 4 where the marker does not count)
constexpr uint32_t LUT_P = 0x00010101u;     // present: r' != 3
constexpr uint32_t SEL_UNUSED = 0x04040404u;

struct FreqArgs {
    const uint32_t* tiles;          // the tile layout as dwords
    int64_t nkb;                    // 256-individual blocks per row group
    int64_t N, M;
    const uint8_t* use;             // M bytes or NULL
    double *mu, *rs;                // nrg * 64 each
    double* zt;                     // nrg * 64 * 4: z[c] of every marker
    uint32_t* kmq;                  // nrg * 16 selector masks
    unsigned long long* tally;      // [0] markers that count, [1] markers selected and dropped (monomorphic or never present)
};

// In the tile layout dword G * 256 + 16 q + p of row group rg holds the individuals 64 G + 4 p + f (field f, 2 bits) at the markers
// 64 rg + 4 q + t (byte t).  Thread (q = tid >> 4, p = tid & 15) walks the groups G: one coalesced KiB per step.
__global__ __launch_bounds__(256) void k_grm_freq(const FreqArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, q = tid >> 4, p = tid & 15;
    const int64_t rg = blockIdx.x, nG = a.nkb * 4;
    const uint32_t* src = a.tiles + rg * a.nkb * 1024 + tid;
    uint32_t n[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0};
    for (int64_t G = 0; G < nG; G++) {
        uint32_t dw = src[G * 256];
        // individuals at or past N do not exist: their fields count as missing, whatever the layout stores there
        const int64_t left = a.N - (G * 64 + 4 * p);
        if (left < 4) dw |= left <= 0 ? 0xFFFFFFFFu : ~(((1u << (2 * (int)left)) - 1u) * 0x01010101u);
        const uint32_t lo = dw & 0x55555555u, hi = (dw >> 1) & 0x55555555u;
        const uint32_t miss = lo & hi, one = lo & ~hi, two = hi & ~lo;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            n[t] += 4u - (uint32_t)__popc((miss >> (8 * t)) & 0xFFu);
            s[t] += (uint32_t)__popc((one >> (8 * t)) & 0xFFu) + 2u * (uint32_t)__popc((two >> (8 * t)) & 0xFFu);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            n[t] += (uint32_t)__shfl_xor((int)n[t], o);
            s[t] += (uint32_t)__shfl_xor((int)s[t], o);
        }
    if (p != 0) return;
    uint32_t w = 0;
    unsigned long long counting = 0, dropped = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int64_t m = rg * 64 + 4 * q + t;
        const bool on = m < a.M && (!a.use || a.use[m] != 0);
        const int64_t nn = n[t], ss = s[t];
        const bool counts = on && nn > 0 && ss > 0 && ss < 2 * nn;
        double mu = 0.0, rs = 0.0;
        if (counts) {
            // THE weights of the contract: these operations, each correctly rounded
            mu = __ddiv_rn((double)ss, (double)nn);
            const double h = __dmul_rn(mu, __dsub_rn(1.0, __dmul_rn(0.5, mu)));
            rs = __ddiv_rn(1.0, __dsqrt_rn(h));
        }
        a.mu[m] = mu;
        a.rs[m] = rs;
        double* z = a.zt + 4 * m;
#pragma unroll
        for (int c = 0; c < 3; c++) z[c] = counts ? __dmul_rn(__dsub_rn((double)c, mu), rs) : 0.0;
        z[3] = 0.0;
        w |= counts ? 0u : (4u << (8 * t));
        counting += counts;
        dropped += on && !counts;
    }
    a.kmq[rg * 16 + q] = w;
    if (counting) atomicAdd(a.tally, counting);
    if (dropped) atomicAdd(a.tally + 1, dropped);
}

struct GrmArgs {
    const uint32_t* tiles;          // the tile layout as dwords
    int64_t nkb, nrg;               // 256-individual blocks per row group; 64-marker row groups
    const double* zt;               // nrg * 256 values z[c] (k_grm_freq)
    const uint32_t* kmq;            // nrg * 16 selector masks (k_grm_freq)
    int64_t N, nG;                  // individuals; groups of 64 of them
    int64_t nblocks;                // blocks of the launch
    const int* blocks;              // EP_RECT: (I, J) of block b, I <= J; EP_PAIRS: NULL, the upper triangle by linear index
    int64_t i0, ni, j0, nj;         // EP_RECT: the rectangle
    double* out;                    // EP_RECT: ni x nj or NULL
    int* mc;                        // EP_RECT: ni x nj or NULL
    double cutoff;                  // EP_PAIRS
    unsigned long long cap;         // EP_PAIRS: slots of the four arrays below
    unsigned long long* found;      // EP_PAIRS: pairs at or above the cutoff (one counter, zeroed before the launch)
    int *pi, *pj;
    double* pa;
    int* pm;
    double* diag;                   // EP_PAIRS: N or NULL
    int* diag_m;                    // EP_PAIRS: N or NULL
    int C;                          // EP_APPLY: columns of the panel, 1 .. GV_GRM_APPLY_MAX_COLS
    const double* w;                // EP_APPLY: the panel, nG * 64 rows of C, zero from row N on
    int64_t a0, ga, b0, gb;         // EP_APPLY: the pass's tile of the block triangle, I in [a0, a0 + ga), J in [b0, b0 + gb)
    double* px;                     // EP_APPLY: block terms (rows of I, source J): [3][gb][ga * 64][C]
    double* py;                     // EP_APPLY: block terms (rows of J, source I): [3][ga][gb * 64][C]; a tile on the diagonal: px
};

enum { EP_RECT, EP_PAIRS, EP_APPLY };

// EP_APPLY: the block's A as an LDS image, NaN where G0 = G1 = G2 = 0 (the diagonal, M_ij = 0, an individual >= N).  A pitch of 65
// doubles = 130 dwords: lane r of a row read (ds_read_b64, banks (a / 4) % 64, two halves of 32 lanes) sits on banks 2 r, 2 r + 1, and a
// transposed read has consecutive lanes on consecutive doubles -- both without a conflict.
constexpr int APPLY_PITCH = 65;

// One block term of gv_grm_apply: lane r is a row of the term, the wave takes the columns wave + 4 k.  Entry (r, j) of the operator's
// block is img[r * sr + j * sj] (sr = pitch, sj = 1: as computed; swapped: the mirror block).  The chain of the contract, literally:
// from +0.0, j ascending, acc = acc + Gp * w with both operations rounded -- written with the plain operators under contract(off): the
// __dadd_rn / __dmul_rn of the headers inherit the translation unit's contraction and would fuse.  A column slot past C runs on column 0
// and is not stored.  Term p of (r, c) goes to dst[p * pstride + r * C + c].
__device__ __forceinline__ void grm_apply_side(const double* img, int sr, int sj, const double* W, int C, int r, int wave, double* dst,
                                               int64_t pstride) {
#pragma clang fp contract(off)
    double t0[8], t1[8], t2[8];
#pragma unroll
    for (int k = 0; k < 8; k++) t0[k] = t1[k] = t2[k] = 0.0;
    const double* e = img + r * sr;
    for (int j = 0; j < 64; j++) {
        const double x = e[j * sj];
        const bool ok = x == x;
        const double g0 = ok ? 1.0 : 0.0, g1 = ok ? x : 0.0;
        const double g2 = g1 * g1;
        const double* wj = W + j * C;
        double wv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) wv[k] = wj[wave + 4 * k < C ? wave + 4 * k : 0];      // (uniform over the wave: scalar loads)
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double m0 = g0 * wv[k], m1 = g1 * wv[k], m2 = g2 * wv[k];
            t0[k] = t0[k] + m0;
            t1[k] = t1[k] + m1;
            t2[k] = t2[k] + m2;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = wave + 4 * k;
        if (c < C) {
            double* d = dst + (int64_t)r * C + c;
            d[0] = t0[k];
            d[pstride] = t1[k];
            d[2 * pstride] = t2[k];
        }
    }
}

// block b of the upper triangle of nG x nG in row-major order (gv_king.hip): row I holds J = I .. nG - 1 and starts at
// I nG - I (I - 1) / 2.  The fp64 estimate of the root is corrected in exact integers.
__device__ __forceinline__ void grm_block_of(int64_t b, int64_t nG, int64_t& I, int64_t& J) {
    const double t = 2.0 * (double)nG + 1.0;
    int64_t i = (int64_t)((t - sqrt(t * t - 8.0 * (double)b)) * 0.5);
    i = i < 0 ? 0 : (i > nG - 1 ? nG - 1 : i);
    while (i > 0 && i * nG - i * (i - 1) / 2 > b) i--;
    while (i + 1 < nG && (i + 1) * nG - (i + 1) * i / 2 <= b) i++;
    I = i;
    J = i + (b - (i * nG - i * (i - 1) / 2));
}

// what one row group needs in LDS
struct GrmStage {
    uint32_t code[2][256];          // [side I, J][16 q + p]: the 2-bit codes of the side's 64 individuals at the 64 markers
    double z[256];                  // [4 marker + c]
    uint32_t km[16];                // the selector mask of quad q
};

template <int EP>
__global__ __launch_bounds__(256, 2) void k_grm_block(const GrmArgs a) {
    // EP_APPLY reuses the staging buffers for the block's image once the K loop is over: 33 KiB a workgroup, so that four workgroups still
    // share a CU's LDS as they do under the other epilogues (the 64 x C slices of the panel are read through the scalar cache instead)
    constexpr size_t kLds = EP == EP_APPLY ? sizeof(double) * 64 * APPLY_PITCH : 2 * sizeof(GrmStage);
    static_assert(kLds >= 2 * sizeof(GrmStage), "the image must cover the staging buffers it replaces");
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLds];
    GrmStage* const stage = reinterpret_cast<GrmStage*>(lds);
    // Workgroups are dealt to the eight XCDs round-robin by block index: XCD x takes a contiguous eighth of the block list, so the
    // workgroups that run side by side on one L2 share their I side (gv_king.hip)
    int64_t b;
    {
        const int64_t q = a.nblocks / 8, r = a.nblocks % 8, x = blockIdx.x % 8, k = blockIdx.x / 8;
        b = x * q + (x < r ? x : r) + k;
    }
    int64_t I, J;
    if constexpr (EP != EP_PAIRS) {
        I = a.blocks[2 * b];
        J = a.blocks[2 * b + 1];
    } else grm_block_of(b, a.nG, I, J);
    if (I < 0 || J >= a.nG || I > J) return;        // (uniform over the workgroup; never true for a list built by the host)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t rgstride = a.nkb * 1024;          // dwords per row group
    const uint32_t* srcI = a.tiles + I * 256 + tid;
    const uint32_t* srcJ = a.tiles + J * 256 + tid;
    v4d acc[2][2];
    v4i cnt[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
            cnt[i][j] = v4i{0, 0, 0, 0};
        }
    // Operand coordinates of this lane within its side's 64 individuals, t = 0, 1 the tile of the wave's 32:
    //   fp64 A and B, i8 B: individual 16 (2 w + t) + lr, natural.
    //   i8 A: row lr of the operand is individual (lr >> 2) + 4 (lr & 3) of the tile, so that register v of lane (lk, .) of the i32
    //   result, row 4 lk + v, is the individual lk + 4 v -- the row of register v of the fp64 result.
    int wI[2], wJ[2], wP[2];        // dword p = individual >> 2 within a quad's 16 dwords
    int sI[2], sJ[2], sP[2];        // 2 (individual & 3): the field's shift
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int ii = 16 * (2 * wr + t) + lr, jj = 16 * (2 * wc + t) + lr, ip = 16 * (2 * wr + t) + (lr >> 2) + 4 * (lr & 3);
        wI[t] = ii >> 2;
        sI[t] = 2 * (ii & 3);
        wJ[t] = jj >> 2;
        sJ[t] = 2 * (jj & 3);
        wP[t] = ip >> 2;
        sP[t] = 2 * (ip & 3);
    }
    uint32_t cI = 0, cJ = 0, km = SEL_UNUSED;
    double zv = 0.0;
    auto fetch = [&](int64_t rg) {
        cI = srcI[rg * rgstride];
        cJ = srcJ[rg * rgstride];
        zv = a.zt[rg * 256 + tid];
        if (tid < 16) km = a.kmq[rg * 16 + tid];
    };
    if (a.nrg > 0) fetch(0);
    for (int64_t rg = 0; rg < a.nrg; rg++) {
        // Two buffers, one barrier: the stores of row group rg + 1 go to the other buffer, and those of rg + 2 come after the barrier of
        // rg + 1, which a wave passes only when it is done reading rg.
        GrmStage& s = stage[rg & 1];
        s.code[0][tid] = cI;
        s.code[1][tid] = cJ;
        s.z[tid] = zv;
        if (tid < 16) s.km[tid] = km;
        if (rg + 1 < a.nrg) fetch(rg + 1);
        __syncthreads();
        // M_ij: one i8 product over the 64 markers.  The lane's 16 K-bytes are the markers 16 lk + [0, 16): quads 4 lk + e.
        {
            v4i Pi[2], Pj[2];
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int q = 4 * lk + e;
                    const uint32_t m = s.km[q];
                    Pi[t][e] = (int)__builtin_amdgcn_perm(0u, LUT_P, ((s.code[0][16 * q + wP[t]] >> sP[t]) & 0x03030303u) | m);
                    Pj[t][e] = (int)__builtin_amdgcn_perm(0u, LUT_P, ((s.code[1][16 * q + wJ[t]] >> sJ[t]) & 0x03030303u) | m);
                }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) cnt[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Pj[j], cnt[i][j], 0, 0, 0);
        }
        // S: K-step kk is quad kk; the lane's operand is marker 4 kk + lk of its individual
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const double* zrow = s.z + 4 * (4 * kk + lk);
            double zi[2], zj[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                zi[t] = zrow[(s.code[0][16 * kk + wI[t]] >> (8 * lk + sI[t])) & 3u];
                zj[t] = zrow[(s.code[1][16 * kk + wJ[t]] >> (8 * lk + sJ[t])) & 3u];
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi[i], zj[j], acc[i][j], 0, 0, 0);
        }
    }
    // Epilogue.  Register v of tile (i, j) of this lane is the pair of individual 16 (2 wr + i) + lk + 4 v of group I and individual
    // 16 (2 wc + j) + lr of group J.  Nothing is emitted for a pad individual (>= N).
    const double nan = __builtin_nan("");
    if constexpr (EP == EP_APPLY) {
        // The block never leaves the workgroup: its image goes to LDS, and every wave then runs the chains of its columns, one lane per
        // row: the term for (rows of I, source J), and off the diagonal the one for (rows of J, source I) from the same image read
        // transposed.  The panel's entry w[j][c] is the same for every lane of a wave: a scalar load.
        double* const img = reinterpret_cast<double*>(lds);
        if (I < a.a0 || I >= a.a0 + a.ga || J < a.b0 || J >= a.b0 + a.gb) return;      // (never true for a list built by the host)
        __syncthreads();                            // every wave is done reading the last row group's staging
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int row = 16 * (2 * wr + i) + lk + 4 * v, col = 16 * (2 * wc + j) + lr;
                    const int64_t gi = I * 64 + row, gj = J * 64 + col;
                    const int mij = cnt[i][j][v];
                    const bool ok = gi < a.N && gj < a.N && gi != gj && mij > 0;
                    img[row * APPLY_PITCH + col] = ok ? __ddiv_rn(acc[i][j][v], (double)mij) : nan;
                }
        __syncthreads();
        const int64_t nw = 64 * a.C, ra = a.ga * 64, rb = a.gb * 64;
        const double *wI = a.w + I * nw, *wJ = a.w + J * nw;
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        grm_apply_side(img, APPLY_PITCH, 1, wJ, a.C, lane, wv, a.px + ((J - a.b0) * ra + (I - a.a0) * 64) * a.C, a.gb * ra * a.C);
        if (I < J) {
            if (a.a0 == a.b0)
                grm_apply_side(img, 1, APPLY_PITCH, wI, a.C, lane, wv, a.px + ((I - a.a0) * ra + (J - a.a0) * 64) * a.C, a.gb * ra * a.C);
            else
                grm_apply_side(img, 1, APPLY_PITCH, wI, a.C, lane, wv, a.py + ((I - a.a0) * rb + (J - a.b0) * 64) * a.C, a.ga * rb * a.C);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int64_t gj = J * 64 + 16 * (2 * wc + j) + lr;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int64_t gi = I * 64 + 16 * (2 * wr + i) + lk + 4 * v;
                if (gi >= a.N || gj >= a.N) continue;
                const int mij = cnt[i][j][v];
                const double A = mij > 0 ? __ddiv_rn(acc[i][j][v], (double)mij) : nan;
                if constexpr (EP == EP_RECT) {
                    // a block off the diagonal also owes the rectangle its mirror image, from the same accumulators
#pragma unroll
                    for (int mir = 0; mir < 2; mir++) {
                        if (mir && I == J) break;
                        const int64_t r = (mir ? gj : gi) - a.i0, c = (mir ? gi : gj) - a.j0;
                        if (r < 0 || r >= a.ni || c < 0 || c >= a.nj) continue;
                        const int64_t o = r * a.nj + c;
                        if (a.out) a.out[o] = A;
                        if (a.mc) a.mc[o] = mij;
                    }
                } else {
                    if (gi == gj) {
                        if (a.diag) a.diag[gi] = A;
                        if (a.diag_m) a.diag_m[gi] = mij;
                    }
                    if (gi < gj && A >= a.cutoff) {         // (a NaN never passes)
                        const unsigned long long slot = atomicAdd(a.found, 1ull);
                        if (slot < a.cap) {
                            a.pi[slot] = (int)gi;
                            a.pj[slot] = (int)gj;
                            a.pa[slot] = A;
                            a.pm[slot] = mij;
                        }
                    }
                }
            }
    }
}

struct ApplyFinishArgs {
    const double* part;             // [3][nsrc][rows][C]: the block terms of one side of a pass
    double* out;                    // [3][nG * 64][C]: the running chains
    int64_t rows, row0, nsrc, N, ostride;
    int C;
};

// extends the chain of every (row, column) of a pass's rows by the pass's source groups in ascending order
__global__ __launch_bounds__(256) void k_grm_apply_finish(const ApplyFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, per = a.rows * a.C;
    if (idx >= per || a.row0 + idx / a.C >= a.N) return;
    for (int p = 0; p < 3; p++) {
        double* o = a.out + p * a.ostride + a.row0 * a.C + idx;
        double acc = *o;
        const double* src = a.part + p * a.nsrc * per + idx;
        for (int64_t s = 0; s < a.nsrc; s++) acc = acc + src[s * per];
        *o = acc;
    }
}

// device scratch of one call: freed when the call returns, however it returns
struct Scratch {
    std::vector<void*> ptrs;
    size_t bytes = 0;
    ~Scratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class T>
    hipError_t get(T** out, size_t n) {
        void* p = nullptr;
        const size_t b = sizeof(T) * (n ? n : 1);
        const hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) return e;
        ptrs.push_back(p);
        bytes += b;
        *out = (T*)p;
        return hipSuccess;
    }
};

// what the pre-pass leaves on the device
struct Weights {
    double *mu = nullptr, *rs = nullptr;
    unsigned long long* tally = nullptr;
};

}  // namespace

using namespace gvi;

// what every entry point needs resident: 2-bit genotypes in the tile layout on a job of one rank.  Neither the phenotype mask nor the
// marker statistics: relatedness is a property of the genotypes.
static int grm_check(gv_ctx* c, const char* who) {
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    REFUSE_DOSAGE(c, who, "the relationship matrix is computed from 2-bit genotypes only");
    if (c->dense.resident)
        return fail(c, "%s: refused for dense (meth) data -- the relationship matrix is computed from 2-bit genotypes only", who);
    if (!c->have_stripes)
        return fail(c, "%s: needs the tile layout resident (gv_set_layout(ctx, .., 2)); raw rows alone are not supported", who);
    if (c->plan.layout != 1 || !c->plan.tiles)
        return fail(c, "%s: two stripe sets are resident, whose individuals are not contiguous per marker group -- upload under the tile layout "
                       "(gv_set_layout(ctx, .., 2))", who);
    if (is_multi(c))
        return fail(c, "%s: a job of more than one rank is refused: S and the common-marker counts are sums over the markers of ALL ranks, "
                       "and the all-reduce that would add them is not built", who);
    if (c->M > GRM_M_MAX)
        return fail(c, "%s: M = %lld exceeds %lld, the most markers whose common-marker count fits its int32 accumulator (1 per marker)", who,
                    (long long)c->M, (long long)GRM_M_MAX);
    return 0;
}

#define GGALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)

// the shared front of the three calls: the argument block and the pre-pass (enqueued, not waited for)
static int grm_prepare(gv_ctx* c, const char* who, const uint8_t* use, Scratch& w, GrmArgs& a, Weights& wt) {
    const gvm::Plan& pl = c->plan;
    a.tiles = reinterpret_cast<const uint32_t*>(pl.tiles);
    a.nkb = pl.nkb_m;
    a.nrg = (c->M + 63) / 64;
    a.N = c->N;
    a.nG = (c->N + 63) / 64;
    const size_t nm = (size_t)a.nrg * 64;
    uint32_t* kmq = nullptr;
    uint8_t* duse = nullptr;
    double* zt = nullptr;
    GGALLOC(kmq, (size_t)a.nrg * 16);
    GGALLOC(zt, 4 * nm);
    GGALLOC(wt.mu, nm);
    GGALLOC(wt.rs, nm);
    GGALLOC(wt.tally, 2);
    if (use) {
        GGALLOC(duse, (size_t)c->M);
        if (c->M > 0) HIPCHK(c, hipMemcpyAsync(duse, use, (size_t)c->M, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(wt.tally, 0, 2 * sizeof(unsigned long long), c->stream));
    if (a.nrg > 0) {
        FreqArgs f{a.tiles, a.nkb, c->N, c->M, duse, wt.mu, wt.rs, zt, kmq, wt.tally};
        hipLaunchKernelGGL(k_grm_freq, dim3((unsigned)a.nrg), dim3(256), 0, c->stream, f);
        KCHK(c);
    }
    a.zt = zt;
    a.kmq = kmq;
    return 0;
}

static void grm_report(gv_ctx* c, std::chrono::steady_clock::time_point t0, int64_t block_pairs, const unsigned long long* tally, int64_t pairs,
                       const Scratch& w) {
    gv_grm_stats& s = c->grm_last;
    s.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    s.block_pairs = block_pairs;
    s.counting_markers = (int64_t)tally[0];
    s.dropped_markers = (int64_t)tally[1];
    s.pairs = pairs;
    s.passes = block_pairs > 0;
    s.blocks_computed = block_pairs;
    s.useful_macs = (double)s.counting_markers * (double)pairs;
    s.scratch_bytes = (double)w.bytes;
}

extern "C" {

int gv_grm_weights(gv_ctx* c, const uint8_t* use, double* mu, double* rs, int64_t* n_used) {
    if (!c) return 1;
    const char* who = "gv_grm_weights";
    if (grm_check(c, who)) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    GrmArgs a{};
    Weights wt;
    if (grm_prepare(c, who, use, w, a, wt)) return 1;
    unsigned long long tally[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(tally, wt.tally, sizeof(tally), hipMemcpyDeviceToHost, c->stream));
    if (mu && c->M > 0) HIPCHK(c, hipMemcpyAsync(mu, wt.mu, sizeof(double) * (size_t)c->M, hipMemcpyDeviceToHost, c->stream));
    if (rs && c->M > 0) HIPCHK(c, hipMemcpyAsync(rs, wt.rs, sizeof(double) * (size_t)c->M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_used) *n_used = (int64_t)tally[0];
    grm_report(c, t0, 0, tally, 0, w);
    return 0;
}

int gv_grm_block(gv_ctx* c, const uint8_t* use, int64_t i0, int64_t ni, int64_t j0, int64_t nj, double* out, int32_t* m_common) {
    if (!c) return 1;
    const char* who = "gv_grm_block";
    if (grm_check(c, who)) return 1;
    if (i0 < 0 || ni < 0 || i0 > c->N - ni || j0 < 0 || nj < 0 || j0 > c->N - nj)
        return fail(c, "%s: the rectangle [%lld, %lld) x [%lld, %lld) is outside [0, N = %lld)", who, (long long)i0, (long long)(i0 + ni),
                    (long long)j0, (long long)(j0 + nj), (long long)c->N);
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    GrmArgs a{};
    Weights wt;
    unsigned long long tally[2] = {0, 0};
    std::vector<int> blocks;
    if (ni > 0 && nj > 0 && (out || m_common)) {
        if (grm_prepare(c, who, use, w, a, wt)) return 1;
        // the blocks (I <= J) that hold an entry of the rectangle or of its mirror image
        const int64_t ra = i0 / 64, rb = (i0 + ni - 1) / 64, ca = j0 / 64, cb = (j0 + nj - 1) / 64;
        for (int64_t I = std::min(ra, ca); I <= std::max(rb, cb); I++)
            for (int64_t J = I; J <= std::max(rb, cb); J++) {
                const bool direct = I >= ra && I <= rb && J >= ca && J <= cb, mirror = J >= ra && J <= rb && I >= ca && I <= cb;
                if (direct || mirror) {
                    blocks.push_back((int)I);
                    blocks.push_back((int)J);
                }
            }
        a.nblocks = (int64_t)blocks.size() / 2;
        if (a.nblocks > GRM_BLOCKS_MAX) return fail(c, "%s: the rectangle spans %lld blocks, more than one launch takes", who, (long long)a.nblocks);
        const size_t ne = (size_t)ni * (size_t)nj;
        int* dblocks = nullptr;
        GGALLOC(dblocks, blocks.size());
        if (out) GGALLOC(a.out, ne);
        if (m_common) GGALLOC(a.mc, ne);
        a.blocks = dblocks;
        a.i0 = i0;
        a.ni = ni;
        a.j0 = j0;
        a.nj = nj;
        HIPCHK(c, hipMemcpyAsync(dblocks, blocks.data(), sizeof(int) * blocks.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_grm_block<EP_RECT>, dim3((unsigned)a.nblocks), dim3(256), 0, c->stream, a);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(tally, wt.tally, sizeof(tally), hipMemcpyDeviceToHost, c->stream));
        if (out) HIPCHK(c, hipMemcpyAsync(out, a.out, sizeof(double) * ne, hipMemcpyDeviceToHost, c->stream));
        if (m_common) HIPCHK(c, hipMemcpyAsync(m_common, a.mc, sizeof(int) * ne, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    grm_report(c, t0, a.nblocks, tally, a.nblocks ? ni * nj : 0, w);
    return 0;
}

int gv_grm_pairs(gv_ctx* c, const uint8_t* use, double cutoff, int64_t cap, int32_t* pi, int32_t* pj, double* av, int32_t* m_common,
                 double* diag, int32_t* diag_m, int64_t* n_found) {
    if (!c) return 1;
    const char* who = "gv_grm_pairs";
    if (grm_check(c, who)) return 1;
    NEED(c, n_found, "gv_grm_pairs: n_found is NULL");
    NEED(c, cap >= 0, "gv_grm_pairs: cap must not be negative");
    NEED(c, cap == 0 || (pi && pj && av && m_common), "gv_grm_pairs: pi, pj, a or m_common is NULL with cap > 0");
    if (std::isnan(cutoff) || cutoff == INFINITY) return fail(c, "gv_grm_pairs: cutoff must be a finite number or -inf (every pair)");
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    GrmArgs a{};
    Weights wt;
    if (grm_prepare(c, who, use, w, a, wt)) return 1;
    const int64_t nG = a.nG;
    a.nblocks = nG * (nG + 1) / 2;
    if (a.nblocks > GRM_BLOCKS_MAX)
        return fail(c, "%s: N = %lld has more than %lld block pairs, the most one launch takes", who, (long long)c->N, (long long)GRM_BLOCKS_MAX);
    a.cutoff = cutoff;
    a.cap = (unsigned long long)cap;
    GGALLOC(a.found, 1);
    GGALLOC(a.pi, (size_t)cap);
    GGALLOC(a.pj, (size_t)cap);
    GGALLOC(a.pa, (size_t)cap);
    GGALLOC(a.pm, (size_t)cap);
    if (diag) GGALLOC(a.diag, (size_t)c->N);
    if (diag_m) GGALLOC(a.diag_m, (size_t)c->N);
    HIPCHK(c, hipMemsetAsync(a.found, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_grm_block<EP_PAIRS>, dim3((unsigned)a.nblocks), dim3(256), 0, c->stream, a);
    KCHK(c);
    unsigned long long found = 0, tally[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&found, a.found, sizeof(found), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tally, wt.tally, sizeof(tally), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> hi, hj, hm;
    std::vector<double> ha;
    if (found > 0 && found <= (unsigned long long)cap) {
        const size_t n = (size_t)found;
        hi.resize(n);
        hj.resize(n);
        hm.resize(n);
        ha.resize(n);
        HIPCHK(c, hipMemcpyAsync(hi.data(), a.pi, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hj.data(), a.pj, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(ha.data(), a.pa, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hm.data(), a.pm, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    }
    // every transfer that can fail comes before the first byte written to the caller
    std::vector<double> hd(diag ? (size_t)c->N : 0);
    std::vector<int> hdm(diag_m ? (size_t)c->N : 0);
    if (diag) HIPCHK(c, hipMemcpyAsync(hd.data(), a.diag, sizeof(double) * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    if (diag_m) HIPCHK(c, hipMemcpyAsync(hdm.data(), a.diag_m, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!hi.empty()) {
        // the slots were handed out in the order the workgroups happened to ask: deliver in ascending (i, j)
        const size_t n = hi.size();
        std::vector<size_t> ord(n);
        std::iota(ord.begin(), ord.end(), (size_t)0);
        std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return hi[x] != hi[y] ? hi[x] < hi[y] : hj[x] < hj[y]; });
        for (size_t t = 0; t < n; t++) {
            const size_t s = ord[t];
            pi[t] = hi[s];
            pj[t] = hj[s];
            av[t] = ha[s];
            m_common[t] = hm[s];
        }
    }
    if (diag) std::copy(hd.begin(), hd.end(), diag);
    if (diag_m) std::copy(hdm.begin(), hdm.end(), diag_m);
    *n_found = (int64_t)found;
    grm_report(c, t0, a.nblocks, tally, c->N * (c->N - 1) / 2, w);
    return 0;
}

// The passes of gv_grm_apply are square tiles of the block triangle, g groups on a side: tile (a, b), a <= b, holds the blocks I in
// group range a, J in range b, and leaves the terms (rows of a, sources of b) and, off the diagonal, (rows of b, sources of a).  Run in
// the order b = 0, 1, ..; a = 0 .. b, the tiles meet every row's sources in ascending order -- (0, a), .., (a, a), (a, a + 1), .. for a row
// of range a -- so the finishing kernel extends the chains pass by pass, and no block is computed twice.
int gv_grm_apply(gv_ctx* c, const uint8_t* use, int C, const double* wh, double* g0, double* g1, double* g2) {
    if (!c) return 1;
    const char* who = "gv_grm_apply";
    if (grm_check(c, who)) return 1;
    if (C < 1 || C > GV_GRM_APPLY_MAX_COLS)
        return fail(c, "%s: C = %d columns is outside 1 .. %d", who, C, GV_GRM_APPLY_MAX_COLS);
    NEED(c, wh, "gv_grm_apply: w is NULL");
    NEED(c, g0 || g1 || g2, "gv_grm_apply: g0, g1 and g2 are all NULL");
    const int64_t N = c->N, nG = (N + 63) / 64, npad = nG * 64;
    for (int64_t t = 0; t < N * C; t++)
        if (!std::isfinite(wh[t]))
            return fail(c, "%s: w[%lld][%lld] is not finite: an absent pair takes part in every sum as 0 * w", who, (long long)(t / C), (long long)(t % C));
    const double unit = 2.0 * 3.0 * 64.0 * (double)C * 8.0;      // both terms of one block
    if (c->grm_part_bytes < unit)
        return fail(c, "%s: the budget of the partial sums, %.0f bytes (GV_GRM_PART_MB), cannot hold the terms of one row group against one "
                       "source group: 2 sides x 3 operators x 64 rows x %d columns x 8 bytes = %.0f bytes", who, c->grm_part_bytes, C, unit);
    if (nG * (nG + 1) / 2 > GRM_BLOCKS_MAX)
        return fail(c, "%s: N = %lld has more than %lld block pairs", who, (long long)N, (long long)GRM_BLOCKS_MAX);
    int64_t g = (int64_t)std::floor(std::sqrt(c->grm_part_bytes / unit));
    while (g > 1 && (double)g * (double)g * unit > c->grm_part_bytes) g--;
    g = std::max<int64_t>(1, std::min(g, nG));
    const int64_t P = (nG + g - 1) / g;
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    GrmArgs a{};
    Weights wt;
    if (grm_prepare(c, who, use, w, a, wt)) return 1;
    // the block lists of all passes, back to back
    std::vector<int> blocks;
    std::vector<int64_t> first;
    blocks.reserve((size_t)(nG * (nG + 1)));
    for (int64_t tb = 0; tb < P; tb++)
        for (int64_t ta = 0; ta <= tb; ta++) {
            first.push_back((int64_t)blocks.size() / 2);
            for (int64_t I = ta * g; I < std::min(nG, (ta + 1) * g); I++)
                for (int64_t J = std::max(I, tb * g); J < std::min(nG, (tb + 1) * g); J++) {
                    blocks.push_back((int)I);
                    blocks.push_back((int)J);
                }
        }
    first.push_back((int64_t)blocks.size() / 2);
    const size_t no = (size_t)npad * (size_t)C, np = 3 * (size_t)(g * g) * 64 * (size_t)C;
    int* dblocks = nullptr;
    double *dw = nullptr, *dout = nullptr;
    GGALLOC(dblocks, blocks.size());
    GGALLOC(dw, no);
    GGALLOC(dout, 3 * no);
    GGALLOC(a.px, np);
    if (P > 1) GGALLOC(a.py, np);
    HIPCHK(c, hipMemcpyAsync(dblocks, blocks.data(), sizeof(int) * blocks.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dw, 0, sizeof(double) * no, c->stream));
    HIPCHK(c, hipMemcpyAsync(dw, wh, sizeof(double) * (size_t)N * (size_t)C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dout, 0, sizeof(double) * 3 * no, c->stream));
    a.C = C;
    a.w = dw;
    int64_t pass = 0;
    for (int64_t tb = 0; tb < P; tb++)
        for (int64_t ta = 0; ta <= tb; ta++, pass++) {
            a.a0 = ta * g;
            a.ga = std::min(nG, (ta + 1) * g) - a.a0;
            a.b0 = tb * g;
            a.gb = std::min(nG, (tb + 1) * g) - a.b0;
            a.blocks = dblocks + 2 * first[(size_t)pass];
            a.nblocks = first[(size_t)pass + 1] - first[(size_t)pass];
            hipLaunchKernelGGL(k_grm_block<EP_APPLY>, dim3((unsigned)a.nblocks), dim3(256), 0, c->stream, a);
            KCHK(c);
            for (int side = 0; side < (ta == tb ? 1 : 2); side++) {
                ApplyFinishArgs f{};
                f.part = side ? a.py : a.px;
                f.out = dout;
                f.rows = (side ? a.gb : a.ga) * 64;
                f.row0 = (side ? a.b0 : a.a0) * 64;
                f.nsrc = side ? a.ga : a.gb;
                f.N = N;
                f.ostride = (int64_t)no;
                f.C = C;
                hipLaunchKernelGGL(k_grm_apply_finish, dim3((unsigned)((f.rows * C + 255) / 256)), dim3(256), 0, c->stream, f);
                KCHK(c);
            }
        }
    // every transfer that can fail comes before the first byte written to the caller
    unsigned long long tally[2] = {0, 0};
    std::vector<double> h(3 * no);
    HIPCHK(c, hipMemcpyAsync(tally, wt.tally, sizeof(tally), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), dout, sizeof(double) * 3 * no, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double* outs[3] = {g0, g1, g2};
    for (int p = 0; p < 3; p++)
        if (outs[p]) std::copy(h.begin() + (size_t)p * no, h.begin() + (size_t)p * no + (size_t)N * (size_t)C, outs[p]);
    grm_report(c, t0, nG * (nG + 1) / 2, tally, N * (N - 1) / 2, w);
    c->grm_last.passes = pass;
    c->grm_last.blocks_computed = (int64_t)blocks.size() / 2;
    return 0;
}

namespace {

// the six sums of the regression and what follows from them; NaN in the derived values when n < 3 or D <= 0
struct HeSums {
    double n, sx, sxx, sz, szz, sxz;
    double h2() const {
        const double D = n * sxx - sx * sx;
        return n >= 3.0 && D > 0.0 ? (n * sxz - sx * sz) / D : std::nan("");
    }
};

}  // namespace

int gv_grm_he(gv_ctx* c, const uint8_t* use, int64_t C, const double* y, gv_he_result* res) {
    if (!c) return 1;
    const char* who = "gv_grm_he";
    if (grm_check(c, who)) return 1;
    if (C < 1) return fail(c, "%s: C = %lld traits: at least one is needed", who, (long long)C);
    NEED(c, y, "gv_grm_he: y is NULL");
    NEED(c, res, "gv_grm_he: res is NULL");
    const int64_t N = c->N;
    for (int64_t t = 0; t < N * C; t++)
        if (std::isinf(y[t]))
            return fail(c, "%s: y[%lld][%lld] is infinite (NaN marks a missing phenotype)", who, (long long)(t / C), (long long)(t % C));
    constexpr int64_t PER = 10;                    // traits of one gv_grm_apply: 3 columns each
    std::vector<gv_he_result> out((size_t)C);
    gv_grm_stats total{};
    for (int64_t c0 = 0; c0 < C; c0 += PER) {
        const int64_t nt = std::min(PER, C - c0), W = 3 * nt;
        std::vector<double> w((size_t)(N * W), 0.0), g[3];
        std::vector<char> usable((size_t)nt, 0);
        for (int64_t t = 0; t < nt; t++) {
            // K, the mean and the variance over it, and the columns k, yt, yt^2
            int64_t nk = 0;
            double sum = 0.0, ss = 0.0;
            for (int64_t i = 0; i < N; i++)
                if (!std::isnan(y[i * C + c0 + t])) {
                    nk++;
                    sum += y[i * C + c0 + t];
                }
            const double m = nk ? sum / (double)nk : 0.0;
            for (int64_t i = 0; i < N; i++)
                if (!std::isnan(y[i * C + c0 + t])) ss += (y[i * C + c0 + t] - m) * (y[i * C + c0 + t] - m);
            const double v = nk > 1 ? ss / (double)(nk - 1) : 0.0, sd = std::sqrt(v);
            usable[(size_t)t] = v > 0.0 && std::isfinite(v) && std::isfinite(1.0 / sd);
            out[(size_t)(c0 + t)].n_ind = nk;
            for (int64_t i = 0; i < N; i++)
                if (!std::isnan(y[i * C + c0 + t])) {
                    const double yt = usable[(size_t)t] ? (y[i * C + c0 + t] - m) / sd : 0.0;      // (a constant trait: k alone)
                    double* row = &w[(size_t)(i * W + 3 * t)];
                    row[0] = 1.0;
                    row[1] = yt;
                    row[2] = yt * yt;
                }
        }
        for (auto& v : g) v.assign((size_t)(N * W), 0.0);
        if (gv_grm_apply(c, use, (int)W, w.data(), g[0].data(), g[1].data(), g[2].data())) return 1;
        total.seconds += c->grm_last.seconds;
        total.passes += c->grm_last.passes;
        total.blocks_computed += c->grm_last.blocks_computed;
        total.useful_macs += c->grm_last.useful_macs;
        total.scratch_bytes = std::max(total.scratch_bytes, c->grm_last.scratch_bytes);
        total.block_pairs = c->grm_last.block_pairs;
        total.counting_markers = c->grm_last.counting_markers;
        total.dropped_markers = c->grm_last.dropped_markers;
        total.pairs = c->grm_last.pairs;
        for (int64_t t = 0; t < nt; t++) {
            gv_he_result& r = out[(size_t)(c0 + t)];
            // row i's share of every sum: u_i (G v)_i; a pair is in two rows, hence the halves
            std::vector<HeSums> row((size_t)N);
            HeSums s{0, 0, 0, 0, 0, 0};
            for (int64_t i = 0; i < N; i++) {
                const size_t o = (size_t)(i * W + 3 * t);
                const double k = w[o], yt = w[o + 1], y2 = w[o + 2];
                HeSums& q = row[(size_t)i];
                q = HeSums{k * g[0][o], k * g[1][o], k * g[2][o], yt * g[0][o + 1], y2 * g[0][o + 2], yt * g[1][o + 1]};
                s.n += q.n;
                s.sx += q.sx;
                s.sxx += q.sxx;
                s.sz += q.sz;
                s.szz += q.szz;
                s.sxz += q.sxz;
            }
            s = HeSums{0.5 * s.n, 0.5 * s.sx, 0.5 * s.sxx, 0.5 * s.sz, 0.5 * s.szz, 0.5 * s.sxz};
            r.n_pairs = (int64_t)s.n;
            r.sum_a = s.sx;
            r.sum_aa = s.sxx;
            r.h2 = usable[(size_t)t] ? s.h2() : std::nan("");
            const double D = s.n * s.sxx - s.sx * s.sx;
            r.intercept = (s.sz - r.h2 * s.sx) / s.n;
            const double rss = s.szz - r.intercept * s.sz - r.h2 * s.sxz;
            r.se_ols = std::sqrt(rss / (s.n - 2.0) * s.n / D);
            if (std::isnan(r.h2)) r.intercept = r.se_ols = std::nan("");
            // the delete-one jackknife: individual i takes its row's terms out of every sum
            double mean = 0.0, dev = 0.0;
            std::vector<double> hj;
            for (int64_t i = 0; i < N; i++)
                if (w[(size_t)(i * W + 3 * t)] != 0.0) {
                    const HeSums& q = row[(size_t)i];
                    hj.push_back(HeSums{s.n - q.n, s.sx - q.sx, s.sxx - q.sxx, s.sz - q.sz, s.szz - q.szz, s.sxz - q.sxz}.h2());
                    mean += hj.back();
                }
            mean /= (double)hj.size();
            for (double v : hj) dev += (v - mean) * (v - mean);
            r.se_jack = std::isnan(r.h2) || hj.empty() ? std::nan("") : std::sqrt((double)(hj.size() - 1) / (double)hj.size() * dev);
        }
    }
    std::copy(out.begin(), out.end(), res);
    c->grm_last = total;
    return 0;
}

int gv_grm_info(gv_ctx* c, gv_grm_stats* info) {
    if (!c || !info) return 1;
    *info = c->grm_last;
    return 0;
}

}  // extern "C"
