// gv_ld.hip -- LD scores and banded LD correlations of the resident genotypes (gv_ld_scores, gv_ld_band), and the
// window Grams of the LD-block preconditioner (gvp::gram; section 13): every exact block of A^T A comes from this file.
//
// C = A^T A restricted to a band of B markers on each side, from the resident 2-bit re-encoding: the exact integer sums VV, VP, PV, PP
// of the planes P = b na, V = a P with v_mfma_i32_16x16x64_i8, then the fixed fp64 combination of section 13 and r = C_jk / sqrt(C_jj C_kk).
//   k_ld_diag    C_jj of every marker from popcounts of the same planes (the same integers an MFMA would sum), one workgroup per
//                64-marker row group
//   k_ld_block   one workgroup per pair of row groups (I, J = I + d), d <= D = (B + 63) / 64: the 64 x 64 block of the four products
//                over all individuals.  Every thread expands the words of one 16-byte load per half K-block into the i8 planes ONCE
//                and shares them through LDS; each of the 4 waves multiplies a 32 x 32 quarter of the block (16 MFMAs per K-step).
//                Epilogue: r, and either the band rows (band mode) or the block's row and column sums of f(r^2) (scores mode); or
//                the block's entries of the preconditioner's window Grams (Gram mode: d only as far as one window reaches, no k_ld_diag)
//   k_ld_finish  l_j = 1 + the 2D + 1 block partials of marker j in ascending block order
// gv_ld_scores_pos (section 19): the band of a marker from its position (hi[], gv_ld_window.h) and scores per annotation category -- the
// EP_POS epilogue of k_ld_block and k_ld_finish_pos, in passes over row groups that keep the partials within a memory budget.
// gv_ld_clump (section 20): LD clumping of association results over the same band -- the EP_ADJ epilogue of k_ld_block thresholds r * r
// into bit words over a list of blocks filtered by eligibility (gv_ld_clump.h), k_clump_round picks the index markers in rounds that
// decide only what is certain, k_clump_assign names every marker's index.
// Integer sums, then a fixed fp64 order, no atomics: the results do not depend on the layout, the kernel mode or the launch.
// Second part (k_ldd_*, ldd_run): the same two entry points on resident 8-bit dosage codes, opt-in (gv_set_ld_dosage; section 17) -- the
// centred product of two markers in exact 128-bit integers, one correctly rounded conversion.  The same block kernel with a Gram epilogue
// builds the preconditioner's window Grams of 8-bit codes (gvp::gram_dosage; section 18).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "gv_internal.h"
#include "gv_ld_clump.h"
#include "gv_ld_window.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// THE int32 invariant of this file: one individual adds at most 2 * 2 = 4 to an int32 sum (VV of two a = 2 genotypes), so a sum over
// all N individuals stays below 2^31 for N <= 2^29 - 1 and no accumulation is cut into segments.  gv_ld_* and the preconditioner's
// Gram build refuse a larger N (planes_check).
constexpr int64_t LD_N_MAX = ((int64_t)1 << 29) - 1;
// ... and of the dosage kernels (k_ldd_block): an individual adds at most 128 * 128 = 16 384 in magnitude to an int32 sum, so no int32
// accumulation spans more than c->dosage_seg <= gvdm::SEG_MAX = 131 071 individuals (GV_DOSAGE_MFMA_SEG lowers it), rounded down to
// whole K-steps of LDD_KSTEP individuals, at least one (ldd_run is the one place that cuts).  The segment sums are added in int64; a
// data set of one segment runs the instantiation without them.  The 128-bit epilogue (ldd_x) holds for N <= LD_N_MAX.
constexpr int LDD_KSTEP = 128;
static_assert((gvdm::SEG_MAX / LDD_KSTEP) * LDD_KSTEP * 128 * 128 <= 2147483647LL, "an int32 sum over one segment must fit");
constexpr int64_t LD_WINDOW_MAX = 8192;
constexpr int LD_PITCH = 65;     // doubles per row of the scores epilogue's 64 x 64 LDS image (odd: row and column walks spread over the banks)
constexpr int ADJ_PITCH = 68;    // bytes per row of the clumping epilogue's 64 x 64 predicate image (17 dwords: a column walk spreads over the banks)

// THE bit recipe of the two integer planes of 16 entries, P = present and phenotyped, V = a P.  w holds r' = 2, 1, 0 for a = 2, 1, 0 and
// 3 for a missing genotype (0 at pad): bit 2q of pm is P of entry q, bits 2q + 1 and 2q of vb are its V.
__device__ __forceinline__ void ld_bits(uint32_t w, uint32_t na, uint32_t& pm, uint32_t& vb) {
    pm = ~(w & (w >> 1)) & na & 0x55555555u;
    vb = w & (pm | (pm << 1));
}

// ... as i8 MFMA operands (VGPR s, byte t = entry 4t + s)
__device__ __forceinline__ void ld_planes(uint32_t w, uint32_t na, v4i& V, v4i& P) {
    uint32_t pm, vb;
    ld_bits(w, na, pm, vb);
#pragma unroll
    for (int s = 0; s < 4; s++) {
        V[s] = (int)((vb >> (2 * s)) & 0x03030303u);
        P[s] = (int)((pm >> (2 * s)) & 0x03030303u);
    }
}

// One 16-byte load of the (row group, K-block) image -- 64 markers x 256 individuals in 256 pieces -- and the four 16-entry words it
// brings.  x in [0, 128) names the piece within half h of the K-block (K-steps 2h and 2h + 1 of 64 individuals); word q belongs to
// marker 16 b[q] + r[q] of the row group and the 16 individuals 16 (4 (2h + sl) + g[q]) + [0, 16) of the K-block.
template <int LAYOUT>
struct Piece {
    // tile layout: piece (s, quad, jj) at s * 64 + quad * 4 + jj holds byte d of marker t of the quad in byte t of dword d: all four
    // markers of the quad, individuals 16 (4 s + jj) + [0, 16)
    // stripes_m:   piece (i, s, r) at i * 64 + s * 16 + r holds marker 16 i + r, individuals 64 s + [0, 64): dword d = 16 of them
    static __device__ __forceinline__ int index(int h, int x) {
        return LAYOUT == 1 ? 128 * h + x : (x >> 5) * 64 + (2 * h + ((x >> 4) & 1)) * 16 + (x & 15);
    }
    static __device__ __forceinline__ int sl(int x) { return LAYOUT == 1 ? x >> 6 : (x >> 4) & 1; }
    static __device__ __forceinline__ int b(int x, int q) { return LAYOUT == 1 ? (x >> 4) & 3 : x >> 5; }
    static __device__ __forceinline__ int r(int x, int q) { return LAYOUT == 1 ? 4 * ((x >> 2) & 3) + q : x & 15; }
    static __device__ __forceinline__ int g(int x, int q) { return LAYOUT == 1 ? x & 3 : q; }
    static __device__ __forceinline__ uint32_t word(const uint4& o, int q) {
        if (LAYOUT == 1) {
            const int sh = 8 * q;
            return ((o.x >> sh) & 0xFFu) | (((o.y >> sh) & 0xFFu) << 8) | (((o.z >> sh) & 0xFFu) << 16) | (((o.w >> sh) & 0xFFu) << 24);
        }
        return q == 0 ? o.x : (q == 1 ? o.y : (q == 2 ? o.z : o.w));
    }
};

// C_jk from the four integer sums: vp = sum V_nj P_nk, pv = sum P_nj V_nk.  THE combination of sections 13 and 16: the LD epilogues call it
// with the lower marker as j, the Gram epilogue with j = the entry's row (the lower triangle of a Gram is what k_pc_factor reads)
__device__ __forceinline__ double ld_c(int vv, int vp, int pv, int pp, double mj, double mk, double sj, double sk, double inv_n) {
    const double s = (double)vv - mk * (double)vp - mj * (double)pv + mj * mk * (double)pp;
    return sj * sk * inv_n * s;
}

// C_jj of the markers of row group blockIdx.x: VV = sum a^2 P, VP = PV = sum a P, PP = sum P by popcount, summed over the threads that
// hold a marker in a fixed order (integers: any order gives the same)
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_ld_diag(const uint4* __restrict__ lay, int64_t nkb, const uint32_t* __restrict__ mask2, int64_t P4,
                                                 int64_t N, int64_t M, const double* __restrict__ mave, const double* __restrict__ msig,
                                                 double* __restrict__ cdiag) {
    __shared__ int red[3][64][16];      // [sum][marker of the row group][slot]
    const int tid = threadIdx.x, h = tid >> 7, x = tid & 127;
    const int64_t rg = blockIdx.x, nJ = (N + 15) / 16, nkbn = (nJ + 15) / 16;
    int vv[4] = {0, 0, 0, 0}, vp[4] = {0, 0, 0, 0}, pp[4] = {0, 0, 0, 0};
    const uint4* p = lay + rg * nkb * 256 + Piece<LAYOUT>::index(h, x);
    for (int64_t kb = 0; kb < nkbn; kb++) {
        const uint4 o = p[kb * 256];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t J = kb * 16 + 4 * (2 * h + Piece<LAYOUT>::sl(x)) + Piece<LAYOUT>::g(x, q);
            const uint32_t na = J < nJ && J < P4 ? mask2[J] : 0u;
            uint32_t pm, vb;
            ld_bits(Piece<LAYOUT>::word(o, q), na, pm, vb);
            const int lo = __popc(vb & 0x55555555u), hi = __popc(vb & 0xAAAAAAAAu);
            vv[q] += lo + 4 * hi;
            vp[q] += lo + 2 * hi;
            pp[q] += __popc(pm);
        }
    }
    // marker ml of the row group is held by 16 (tile layout: 2 h x 2 sl x 4 jj, word q = ml % 4) or 4 x 4 (stripes: 2 h x 2 sl threads,
    // all four words) partial sums: slot = the holder's index among them
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int ml = 16 * Piece<LAYOUT>::b(x, q) + Piece<LAYOUT>::r(x, q);
        const int slot = LAYOUT == 1 ? (h * 2 + Piece<LAYOUT>::sl(x)) * 4 + (x & 3) : (h * 2 + Piece<LAYOUT>::sl(x)) * 4 + q;
        red[0][ml][slot] = vv[q];
        red[1][ml][slot] = vp[q];
        red[2][ml][slot] = pp[q];
    }
    __syncthreads();
    if (tid < 64) {
        const int64_t j = rg * 64 + tid;
        int s[3] = {0, 0, 0};
#pragma unroll
        for (int t = 0; t < 3; t++)
            for (int e = 0; e < 16; e++) s[t] += red[t][tid][e];
        if (j < M) cdiag[j] = ld_c(s[0], s[1], s[1], s[2], mave[j], mave[j], msig[j], msig[j], 1.0 / (double)N);
    }
}

struct LdArgs {
    const uint4* lay;
    int64_t nkb;
    const uint32_t* mask2;
    int64_t P4, N, M, B;
    int64_t nrg, I0;                // row groups in all; the first row group of this launch (band mode starts at the requested rows)
    const double *mave, *msig, *cdiag;
    const int* chrom;               // M device ints or NULL
    int adjusted;
    double nm2;                     // nonas - 2
    int D;                          // (B + 63) / 64
    int64_t Mp;                     // scores: markers per slot of the partials, 64 nrg
    double* part;                   // scores: (2D + 1) x Mp partial sums, slot D + (other row group - own row group)
    int* pcnt;                      // scores: ... and the number of terms in each
    int64_t j0, nj;                 // band: the requested rows
    double* band;                   // band: nj x (2B + 1)
    int64_t S, u0, nu;              // Gram: the shard's first global marker; the half-grid windows [u0, u0 + nu) that overlap it
    int W, hs;                      // Gram: the window length and log2 of its half H
    double* gram;                   // Gram: nu x W x W, zeroed before the launch
    // positional scores (EP_POS, section 19).  The launch covers the row groups of one pass, the first of them I0; its partials are laid
    // out by the block that writes them: row sums [I - I0][d = J - I in 0..dmax][64][ncat] in part / pcnt (pcnt without ncat), column
    // sums (the terms the block owes the markers of J, d >= 1) [I - I0][d - 1][64][ncat] in cpart / ccnt
    const int64_t* hi;              // M: the last in-band index of every marker (gv_ld_window.h)
    const double* annot;            // M x ncat row-major or NULL (one category, a = 1)
    int ncat, dmax;
    double* cpart;
    int* ccnt;
    const int* pairs;               // the blocks of the launch, (I, J) of block blockIdx.x: a 1-D grid over the blocks that hold an in-band pair
    // clumping (EP_ADJ, section 20): hi, dmax and pairs as above
    const int* crank;               // M: the rank of a marker of E2 in the order of (p, index), -1 outside E2 (gv_ld_clump.h)
    double r2;                      // the threshold on r * r
    uint64_t* adjw;                 // [nrg][2 dmax + 1][64] adjacency words, slot dmax + (other row group - own), zeroed before the launch
};

enum { EP_SCORES, EP_BAND, EP_GRAM, EP_POS, EP_ADJ };     // the epilogues of k_ld_block

// f(r^2) of the LD score
__device__ __forceinline__ double ld_f(double r, int adjusted, double nm2) {
    const double x = r * r;
    return adjusted ? x - (1.0 - x) / nm2 : x;
}

// s + f a of the positional scores: the plain product, then the sum (the contract of gv_ld_scores_pos: never contracted into an fma)
__device__ __forceinline__ double ld_term_add(double s, double f, double a) {
#pragma clang fp contract(off)
    const double p = f * a;
    return s + p;
}

// The EP_POS epilogue after the block's 64 x 64 image of f(r^2) (NaN = no term) is in LDS: for every category c the rows of I times the
// annotation rows of J, out[e][c] = sum_t f[e][t] a[64 J + t][c] in ascending t, and for I < J the columns times the annotation rows of
// I.  The (row or column, e, c) triples are dealt to the 256 threads with c fastest: the annotation reads and the store coalesce along c,
// the LDS reads are broadcasts.  With one category these are the 128 threads of the EP_SCORES epilogue.  An annotation row past M is
// never read: t stops at M.  The annotation value of every t < tn is loaded whether its f is a term or not, so that the loads do not
// hang on the NaN test and the compiler can issue a batch of them ahead of the sums (eight, the unroll); the sum takes the terms alone,
// in order.  The term counts are written once per marker, by the thread of c = 0.
__device__ __forceinline__ void ld_pos_sums(const LdArgs& a, const double* fl, int64_t I, int64_t J, int tid) {
    const int C = a.ncat, d = (int)(J - I);
    const int64_t Il = I - a.I0;
    const int nq = (I == J ? 64 : 128) * C;
    for (int q = tid; q < nq; q += 256) {
        const bool col = q >= 64 * C;
        const int p = col ? q - 64 * C : q;
        const int e = p / C, c = p - e * C;
        const int64_t other = (col ? I : J) * 64;
        const int tn = (int)min((int64_t)64, a.M - other);
        const double* an = a.annot ? a.annot + other * C + c : nullptr;
        double s = 0.0;
        int n = 0;
#pragma unroll 8
        for (int t = 0; t < tn; t++) {
            const double f = col ? fl[t * LD_PITCH + e] : fl[e * LD_PITCH + t];
            const double av = an ? an[(int64_t)t * C] : 1.0;
            const bool term = f == f;
            s = term ? ld_term_add(s, f, av) : s;
            n += term;
        }
        const int64_t slot = (col ? Il * a.dmax + (d - 1) : Il * (a.dmax + 1) + d) * 64;
        (col ? a.cpart : a.part)[slot * C + p] = s;
        if (c == 0) (col ? a.ccnt : a.pcnt)[slot + e] = n;
    }
}

// G_u[m - lo_u][k - lo_u] = g and, if mirror, G_u[k - lo_u][m - lo_u] = gt in every half-grid window u = [(u - 1) H, (u + 1) H) that holds
// the local markers m and k: with am = (S + m) / H and ak = (S + k) / H, u = am and am + 1 if am == ak, the larger if they differ by 1.
// (lo_u <= m, k < lo_u + W because both markers lie in the window; u0 <= am and ak + 1 < u0 + nu for m, k < M.)
// (A: LdArgs or LddArgs -- the window fields S, u0, nu, W, hs, gram of either)
template <class A>
__device__ __forceinline__ void ld_gram_store(const A& a, int64_t m, int64_t k, double g, bool mirror, double gt) {
    const int64_t am = (a.S + m) >> a.hs, ak = (a.S + k) >> a.hs;
    for (int64_t u = max(am, ak); u <= min(am, ak) + 1; u++) {
        if (u < a.u0 || u >= a.u0 + a.nu) continue;
        const int64_t lo = max((u - 1) * ((int64_t)1 << a.hs), a.S) - a.S;
        double* G = a.gram + (u - a.u0) * a.W * a.W;
        const int r = (int)(m - lo), c = (int)(k - lo);
        G[r * a.W + c] = g;
        if (mirror) G[c * a.W + r] = gt;
    }
}

// block (I = I0 + blockIdx.x, J = I + blockIdx.y).  EP_BAND: store r of the requested rows; EP_SCORES: the block's row / column sums;
// EP_GRAM: the block's entries of the window Grams; EP_POS: the band is k <= hi[m] (section 19), the block's row / column sums per
// annotation category; the launch is a 1-D grid over a host-built list of the blocks that hold an in-band pair.  EP_ADJ (section 20): the
// band and the list of EP_POS, r of EP_BAND; the block's 64 x 64 adjacency predicate as 64 row words and, for I < J, 64 column words.
template <int LAYOUT, int EP>
__global__ __launch_bounds__(256) void k_ld_block(const LdArgs a) {
    // operand images of one half K-block: [side: I, J][16-marker tile][K-step of the half][plane V, P][lane] x 16 bytes = 32 KiB;
    // the scores epilogue reuses the space for the block's 64 x 64 values of f(r^2)
    constexpr int OP_BYTES = 2 * 4 * 2 * 2 * 64 * 16, EP_BYTES = 64 * LD_PITCH * 8;
    constexpr bool LD = EP != EP_GRAM;      // r needs the diagonal and the chromosomes; a Gram entry neither
    constexpr bool POSW = EP == EP_POS || EP == EP_ADJ;     // the band by hi[] over the list of blocks
    constexpr bool CH = LD && !POSW;            // (the positional band has the chromosomes folded into hi)
    __shared__ __attribute__((aligned(16))) char lds[(EP == EP_SCORES || EP == EP_POS) && EP_BYTES > OP_BYTES ? EP_BYTES : OP_BYTES];
    v4i* op = reinterpret_cast<v4i*>(lds);
    int64_t I = a.I0 + blockIdx.x, J = I + blockIdx.y;
    if constexpr (POSW) {
        I = a.pairs[2 * blockIdx.x];
        J = a.pairs[2 * blockIdx.x + 1];
    }
    if (I >= a.nrg || J >= a.nrg) return;       // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int side = tid >> 7, x = tid & 127;
    const int64_t nJ = (a.N + 15) / 16, nkbn = (nJ + 15) / 16;
    v4i acc[4][2][2];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[p][i][j] = v4i{0, 0, 0, 0};
    const uint4* src = a.lay + (side ? J : I) * a.nkb * 256;
    const int psl = Piece<LAYOUT>::sl(x);
    const int64_t steps = 2 * nkbn;              // half K-blocks
    // this thread's piece of half K-block st and the mask words of its four words, loaded one step ahead of their use
    uint4 o;
    uint32_t na[4];
    auto fetch = [&](int64_t st) {
        const int64_t kb = st >> 1;
        const int h = (int)(st & 1);
        o = src[kb * 256 + Piece<LAYOUT>::index(h, x)];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t Jn = kb * 16 + 4 * (2 * h + psl) + Piece<LAYOUT>::g(x, q);
            na[q] = Jn < nJ && Jn < a.P4 ? a.mask2[Jn] : 0u;
        }
    };
    fetch(0);
    for (int64_t st = 0; st < steps; st++) {
        // expand the four words once, for the whole workgroup
#pragma unroll
        for (int q = 0; q < 4; q++) {
            v4i V, P;
            ld_planes(Piece<LAYOUT>::word(o, q), na[q], V, P);
            const int slot = (((side * 4 + Piece<LAYOUT>::b(x, q)) * 2 + psl) * 2) * 64 + Piece<LAYOUT>::g(x, q) * 16 + Piece<LAYOUT>::r(x, q);
            op[slot] = V;
            op[slot + 64] = P;
        }
        if (st + 1 < steps) fetch(st + 1);
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < 2; sl++) {
            v4i Vi[2], Pi[2], Vj[2], Pj[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int si = (((0 * 4 + 2 * wr + t) * 2 + sl) * 2) * 64 + lane, sj = (((1 * 4 + 2 * wc + t) * 2 + sl) * 2) * 64 + lane;
                Vi[t] = op[si];
                Pi[t] = op[si + 64];
                Vj[t] = op[sj];
                Pj[t] = op[sj + 64];
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Vi[i], Vj[j], acc[0][i][j], 0, 0, 0);   // VV
                    acc[1][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Vi[i], Pj[j], acc[1][i][j], 0, 0, 0);   // VP_ik = sum V_ni P_nk
                    acc[2][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Vj[j], acc[2][i][j], 0, 0, 0);   // VP_ki
                    acc[3][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Pj[j], acc[3][i][j], 0, 0, 0);   // PP
                }
        }
        __syncthreads();
    }
    // Epilogue.  Register v of tile (i, j) of this lane is the entry of row 16 (2 wr + i) + 4 (lane >> 4) + v, column
    // 16 (2 wc + j) + (lane & 15) of the block.
    const double inv_n = 1.0 / (double)a.N;
    double* fl = reinterpret_cast<double*>(lds);
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int kl = 16 * (2 * wc + j) + (lane & 15);
        const int64_t k = J * 64 + kl;
        const bool kin = k < a.M;
        const double mk = kin ? a.mave[k] : 0.0, sk = kin ? a.msig[k] : 0.0, ck = LD && kin ? a.cdiag[k] : 0.0;
        const int chk = CH && kin && a.chrom ? a.chrom[k] : 0;
        int64_t hik = 0;
        if constexpr (POSW) hik = kin ? a.hi[k] : 0;
        bool ek = false;
        if constexpr (EP == EP_ADJ) ek = kin && a.crank[k] >= 0;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int il = 16 * (2 * wr + i) + 4 * (lane >> 4) + v;
                const int64_t m = I * 64 + il;
                const bool min_ = m < a.M;
                const double mi = min_ ? a.mave[m] : 0.0, si = min_ ? a.msig[m] : 0.0, ci = LD && min_ ? a.cdiag[m] : 0.0;
                const int chi = CH && min_ && a.chrom ? a.chrom[m] : 0;
                if (EP == EP_GRAM) {
                    // the roles go by the entry's row and column (G[row][col] takes mave_col with sum V_row P_col), so the mirror
                    // image swaps them.  A diagonal block holds both orders itself.
                    if (min_ && kin)
                        ld_gram_store(a, m, k, ld_c(acc[0][i][j][v], acc[1][i][j][v], acc[2][i][j][v], acc[3][i][j][v], mi, mk, si, sk, inv_n), I != J,
                                      ld_c(acc[0][i][j][v], acc[2][i][j][v], acc[1][i][j][v], acc[3][i][j][v], mk, mi, sk, si, inv_n));
                    continue;
                }
                const int64_t dist = k - m;
                bool inband;
                if constexpr (POSW) {
                    const int64_t him = min_ ? a.hi[m] : 0;
                    inband = min_ && kin && (m <= k ? k <= him : m <= hik);      // (k <= hi_m <=> m >= lo_k)
                }
                else inband = min_ && kin && dist <= a.B && -dist <= a.B && chi == chk;
                const bool poly = ci != 0.0 && ck != 0.0;
                double r = 0.0;
                if (inband && poly) {
                    if (m == k) r = 1.0;
                    else {
                        // once per unordered pair: the lower marker takes the role of j (only the diagonal block holds m > k)
                        const double c = m < k ? ld_c(acc[0][i][j][v], acc[1][i][j][v], acc[2][i][j][v], acc[3][i][j][v], mi, mk, si, sk, inv_n)
                                               : ld_c(acc[0][i][j][v], acc[2][i][j][v], acc[1][i][j][v], acc[3][i][j][v], mk, mi, sk, si, inv_n);
                        r = c / sqrt(m < k ? ci * ck : ck * ci);
                    }
                }
                if (EP == EP_BAND) {
                    if (inband) {
                        const int64_t w = 2 * a.B + 1;
                        if (m >= a.j0 && m < a.j0 + a.nj) a.band[(m - a.j0) * w + a.B + dist] = r;
                        if (I != J && k >= a.j0 && k < a.j0 + a.nj) a.band[(k - a.j0) * w + a.B - dist] = r;     // the mirror image
                    }
                } else if constexpr (EP == EP_ADJ) {
                    // adj(m, k): in the band, not the marker itself, both polymorphic, both in E2, r * r >= r2 on the bits of EP_BAND
                    const bool em = min_ && a.crank[m] >= 0;
                    reinterpret_cast<unsigned char*>(lds)[il * ADJ_PITCH + kl] = inband && poly && m != k && em && ek && r * r >= a.r2;
                } else {
                    // a term of l_m (and, mirrored, of l_k): in the band, not the marker itself, both polymorphic; NaN = no term
                    fl[il * LD_PITCH + kl] = inband && poly && m != k ? ld_f(r, a.adjusted, a.nm2) : __builtin_nan("");
                }
            }
    }
    if constexpr (EP == EP_POS) {
        __syncthreads();
        ld_pos_sums(a, fl, I, J, tid);
        return;
    }
    if constexpr (EP == EP_ADJ) {
        __syncthreads();
        // wave w forms the words of the rows and of the columns 16 w + [0, 16): one wave64 ballot per word, lane t voting bit t.  Lane i
        // keeps row word i, lane 16 + i column word i, and the 16 (or 32) lanes store them side by side.
        const unsigned char* pb = reinterpret_cast<const unsigned char*>(lds);
        uint64_t word = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int e = 16 * wave + i;
            const uint64_t rw = __ballot(pb[e * ADJ_PITCH + lane] != 0), cw = __ballot(pb[lane * ADJ_PITCH + e] != 0);
            if (lane == i) word = rw;
            if (lane == 16 + i) word = cw;
        }
        const int64_t nsl = 2 * a.dmax + 1, d = J - I;
        if (lane < 16) a.adjw[((I * nsl + a.dmax + d) * 64) + 16 * wave + lane] = word;
        else if (lane < 32 && I != J) a.adjw[((J * nsl + a.dmax - d) * 64) + 16 * wave + lane - 16] = word;
        return;
    }
    if (EP != EP_SCORES) return;
    __syncthreads();
    // rows of I summed over the columns in ascending k (threads 0..63); columns of J over the rows in ascending order (64..127, I < J)
    if (tid < 128 && (tid < 64 || I != J)) {
        const bool col = tid >= 64;
        const int e = tid & 63;
        double s = 0.0;
        int n = 0;
        for (int t = 0; t < 64; t++) {
            const double f = col ? fl[t * LD_PITCH + e] : fl[e * LD_PITCH + t];
            if (f == f) {
                s += f;
                n++;
            }
        }
        const int64_t m = (col ? J : I) * 64 + e;
        const int64_t slot = col ? a.D - (J - I) : a.D + (J - I);
        a.part[slot * a.Mp + m] = s;          // (m < Mp = 64 nrg: the rows past M hold 0 terms)
        a.pcnt[slot * a.Mp + m] = n;
    }
}

// l_j = 1 + the block partials of marker j in ascending block order (slots whose block does not exist were zeroed)
__global__ __launch_bounds__(256) void k_ld_finish(const double* __restrict__ part, const int* __restrict__ pcnt, int nslots, int64_t Mp,
                                                   int64_t M, const double* __restrict__ cdiag, double* __restrict__ l2,
                                                   double* __restrict__ npairs) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    if (cdiag[j] == 0.0) {
        l2[j] = __builtin_nan("");
        npairs[j] = 0.0;
        return;
    }
    double s = 0.0;
    int64_t n = 0;
    for (int t = 0; t < nslots; t++) {
        s += part[(int64_t)t * Mp + j];
        n += pcnt[(int64_t)t * Mp + j];
    }
    l2[j] = 1.0 + s;
    npairs[j] = (double)(1 + n);
}

// The finish of one pass [Ia, Ib] of the positional scores, thread (j, c) with c fastest over the markers of the row groups
// [Ia, min(Ib + dmax, nrg - 1)]: the running sum run[j][c] (zero before the first pass) takes the pass's partials of marker j in
// ascending block order -- the column sums of the blocks (I, R), I < R, then the row sums of (R, R + d) -- and a marker whose own row
// group R lies in the pass has seen every block: the self term a_jc is added last, as k_ld_finish adds the 1.  A marker of a later row
// group is taken up again by the next pass where this one stopped, so the order of the additions does not depend on the passes.
__global__ __launch_bounds__(256) void k_ld_finish_pos(const double* __restrict__ part, const int* __restrict__ pcnt,
                                                       const double* __restrict__ cpart, const int* __restrict__ ccnt, int dmax, int C,
                                                       int64_t Ia, int64_t Ib, int64_t nrg, int64_t M, const double* __restrict__ cdiag,
                                                       const double* __restrict__ annot, double* __restrict__ run, double* __restrict__ nrun) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, jl = t / C;
    const int c = (int)(t - jl * C);
    const int64_t j = Ia * 64 + jl, R = j >> 6;
    if (j >= M || R > Ib + dmax) return;
    const int e = (int)(j & 63);
    const bool last = R <= Ib;
    if (cdiag[j] == 0.0) {
        if (last) {
            run[j * C + c] = __builtin_nan("");
            if (c == 0) nrun[j] = 0.0;
        }
        return;
    }
    double s = run[j * C + c];
    int64_t n = 0;
    for (int64_t I = max(Ia, R - dmax); I <= min(R - 1, Ib); I++) {
        const int64_t slot = ((I - Ia) * dmax + (R - I - 1)) * 64 + e;
        s += cpart[slot * C + c];
        n += ccnt[slot];
    }
    if (last)
        for (int d = 0; d <= dmax; d++) {
            const int64_t slot = ((R - Ia) * (dmax + 1) + d) * 64 + e;
            s += part[slot * C + c];
            n += pcnt[slot];
        }
    if (last) {
        s = (annot ? annot[j * C + c] : 1.0) + s;
        n++;
    }
    run[j * C + c] = s;
    if (c == 0) nrun[j] += (double)n;
}

// The selection of the index markers (section 20).  state[j]: UNDECIDED, INDEX or CLAIMED, written once.  The words of marker j are the
// 2 dmax + 1 slots adjw[j / 64][.][j % 64]; bit t of slot s names marker 64 (j / 64 + s - dmax) + t (a slot whose row group does not
// exist was never written: zero).
enum { CL_UNDECIDED = 0, CL_INDEX = 1, CL_CLAIMED = 2 };

// One round, thread q for the marker of rank q (the markers of E1 are the ranks [0, n_e1)): still undecided, it becomes claimed if a
// neighbour of lower rank is an index, an index if every neighbour of lower rank is claimed, and waits otherwise -- a decision is taken
// only when no later state of a neighbour can change it, so a neighbour's state read while its thread writes it gives the same end.  (A
// neighbour of lower rank is in E1 itself.)  left counts the markers that wait.
__global__ __launch_bounds__(256) void k_clump_round(const uint64_t* __restrict__ adjw, const int* __restrict__ order, const int* __restrict__ crank,
                                                     int64_t n_e1, int dmax, int64_t nrg, int* state, int* __restrict__ left) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_e1) return;
    const int64_t j = order[q], R = j >> 6;
    if (__atomic_load_n(&state[j], __ATOMIC_RELAXED) != CL_UNDECIDED) return;
    const int nsl = 2 * dmax + 1;
    const uint64_t* w = adjw + (R * nsl) * 64 + (j & 63);
    bool wait = false;
    for (int s = 0; s < nsl; s++) {
        const int64_t Rk = R + s - dmax;
        if (Rk < 0 || Rk >= nrg) continue;
        uint64_t bits = w[(int64_t)s * 64];
        while (bits) {
            const int t = __builtin_ctzll(bits);
            bits &= bits - 1;
            const int64_t k = Rk * 64 + t;
            if (crank[k] >= q) continue;
            const int st = __atomic_load_n(&state[k], __ATOMIC_RELAXED);
            if (st == CL_INDEX) {
                __atomic_store_n(&state[j], (int)CL_CLAIMED, __ATOMIC_RELAXED);
                return;
            }
            wait |= st == CL_UNDECIDED;
        }
    }
    if (wait) atomicAdd(left, 1);
    else __atomic_store_n(&state[j], (int)CL_INDEX, __ATOMIC_RELAXED);
}

// index_of of every marker once no marker of E1 is undecided: -1 outside E2, itself for an index, else the index of the lowest rank
// among its neighbours, else -1
__global__ __launch_bounds__(256) void k_clump_assign(const uint64_t* __restrict__ adjw, const int* __restrict__ crank, const int* __restrict__ state,
                                                      int dmax, int64_t nrg, int64_t M, int64_t* __restrict__ index_of) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    int64_t out = -1;
    if (crank[j] >= 0) {
        if (state[j] == CL_INDEX) out = j;
        else {
            const int nsl = 2 * dmax + 1;
            const int64_t R = j >> 6;
            const uint64_t* w = adjw + (R * nsl) * 64 + (j & 63);
            int best = 0x7FFFFFFF;
            for (int s = 0; s < nsl; s++) {
                const int64_t Rk = R + s - dmax;
                if (Rk < 0 || Rk >= nrg) continue;
                uint64_t bits = w[(int64_t)s * 64];
                while (bits) {
                    const int t = __builtin_ctzll(bits);
                    bits &= bits - 1;
                    const int64_t k = Rk * 64 + t;
                    if (state[k] == CL_INDEX && crank[k] < best) {
                        best = crank[k];
                        out = k;
                    }
                }
            }
        }
    }
    index_of[j] = out;
}

// =====================================================================================================================================
// 8-bit dosage codes (gv_set_ld_dosage).  The operands are the resident pitched rows as they are: byte code ^ 0x80
// is the i8 value code - 128, and 16 consecutive bytes of a row are a lane's share of an MFMA operand on either side.
//   k_ldd_mask   the phenotype mask as one byte per individual (0xFF / 0), zero from N up to the padded length: what the J side is
//                ANDed with.  na is 0 or 1, so masking ONE side masks every product; pad bytes (code 0, -128 after the bias) and whatever
//                a clamped load brings on the other side multiply zeros.
//   k_ldd_diag   c_j = sum P_j, T_j = sum V_j, VV_jj and fl(X_jj) per marker in one streaming read, one wave per marker
//   k_ldd_block  one workgroup per pair of groups of EDGE markers (I, I + d): K-steps of 128 individuals staged once per workgroup in LDS
//                in operand order; wave (wr, wc) multiplies the EDGE/2 x EDGE/2 quarter.  UNIFORM (every marker has P_j = na): one
//                product, VV; otherwise the four products of the bed kernel.  Both feed ldd_x, the ONE epilogue function.
// The epilogue works per 64 x 64 sub-block (Is, Js) of the block, so the partials layout [2D + 1][64 row groups], the summation order and
// k_ld_finish are those of the bed kernel whatever EDGE is.
constexpr uint32_t LDD_BIAS = 0x80808080u;

// 0xFF in every byte of x that is not the reserved code 255
__device__ __forceinline__ uint32_t ldd_present(uint32_t x) {
    const uint32_t miss = ((x & 0x7F7F7F7Fu) + 0x01010101u) & x & 0x80808080u;      // bit 7 of every byte that is 0xFF
    return ~((miss >> 7) * 0xFFu);
}

// a 128-bit integer to fp64, correctly rounded: the top 64 bits with a sticky bit ORed into bit 0 (53 kept bits and the rounding bit
// lie above it), converted as uint64 (one rounding), then scaled by a power of two
__device__ __forceinline__ double ldd_to_double(__int128 x) {
    const bool neg = x < 0;
    const unsigned __int128 u = neg ? -(unsigned __int128)x : (unsigned __int128)x;
    const uint64_t hi = (uint64_t)(u >> 64), lo = (uint64_t)u;
    double d;
    if (hi == 0) d = (double)lo;
    else {
        const int sh = 64 - __builtin_clzll(hi);        // 1 .. 64 bits dropped
        const uint64_t top = sh == 64 ? hi : (hi << (64 - sh)) | (lo >> sh);
        const bool sticky = sh == 64 ? lo != 0 : (lo << (64 - sh)) != 0;
        d = ldexp((double)(top | (uint64_t)sticky), sh);
    }
    return neg ? -d : d;
}

// THE epilogue function of section 17: fl(X_jk), X_jk = c_j c_k VV - c_j T_k VP_jk - c_k T_j VP_kj + T_j T_k PP in exact integers
// (|X| < 2^103 for N <= LD_N_MAX: every factor pair and every sum fits 128 bits).  X_jk = X_kj exactly: no role of j and k enters.
__device__ __forceinline__ double ldd_x(int64_t cj, int64_t ck, int64_t tj, int64_t tk, int64_t vv, int64_t vpjk, int64_t vpkj, int64_t pp) {
    typedef __int128 i128;
    const i128 x = (i128)cj * ck * vv - (i128)cj * tk * vpjk - (i128)ck * tj * vpkj + (i128)tj * tk * pp;
    return ldd_to_double(x);
}

// nab[w]: the mask bytes of the individuals 4 w + [0, 4)
__global__ __launch_bounds__(256) void k_ldd_mask(const uint32_t* __restrict__ mask2, int64_t P4, int64_t N, int64_t nwords,
                                                  uint32_t* __restrict__ nab) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    uint32_t out = 0;
    const int64_t Jn = w >> 2;
    if (Jn < P4) {
        const uint32_t m = mask2[Jn] >> (8 * (w & 3));
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (4 * w + t < N && ((m >> (2 * t)) & 1u)) out |= 0xFFu << (8 * t);
    }
    nab[w] = out;
}

__device__ __forceinline__ int64_t ldd_wave_sum(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor((long long)v, off, 64);
    return v;
}

// one wave per marker; a lane adds the 16 bytes of a load in int32 (at most 16 * 16384) and keeps its running sums in int64
template <bool NA>
__global__ __launch_bounds__(256) void k_ldd_diag(const uint8_t* __restrict__ rows, int64_t pitch, const uint4* __restrict__ nab, int64_t M,
                                                  int64_t* __restrict__ cnt, int64_t* __restrict__ tsum, int64_t* __restrict__ vvd,
                                                  double* __restrict__ xd) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= M) return;
    const uint4* row = reinterpret_cast<const uint4*>(rows + j * pitch);
    int64_t c = 0, t = 0, vv = 0;
    for (int64_t q = lane; q < pitch / 16; q += 64) {
        const uint4 o = row[q], nm = nab[q];
        const uint32_t ow[4] = {o.x, o.y, o.z, o.w}, mw[4] = {nm.x, nm.y, nm.z, nm.w};
        int c1 = 0, t1 = 0, v1 = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t m = NA ? mw[d] & ldd_present(ow[d]) : mw[d];
            const uint32_t v = (ow[d] ^ LDD_BIAS) & m;
            c1 += __popc(m & 0x01010101u);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int s = (int)(signed char)(v >> (8 * b));
                t1 += s;
                v1 += s * s;
            }
        }
        c += c1;
        t += t1;
        vv += v1;
    }
    c = ldd_wave_sum(c);
    t = ldd_wave_sum(t);
    vv = ldd_wave_sum(vv);
    if (lane == 0) {
        cnt[j] = c;
        tsum[j] = t;
        vvd[j] = vv;
        xd[j] = ldd_x(c, c, t, t, vv, t, t, c);        // VP_jj = sum V_j P_j = T_j, PP_jj = c_j
    }
}

struct LddArgs {
    const uint8_t* rows;
    int64_t pitch;
    const uint4* nab;               // mask bytes, 16 individuals per element, steps * 8 elements
    int64_t N, M, B, nonas;
    int64_t steps, seg_steps;       // K-steps of 128 individuals in all; per int32 segment (SEGMENTED only)
    int64_t nrg, nrge, I0;          // 64-marker row groups; groups of EDGE markers; the first of those of this launch
    const int64_t *cnt, *tsum;
    const double* xd;               // fl(X_jj): 0 = monomorphic
    const int* chrom;
    int adjusted;
    double nm2;
    int D;
    int64_t Mp;
    double* part;
    int* pcnt;
    int64_t j0, nj;
    double* band;
    const double* msig;             // Gram: the marker statistics; s_j = msig_j * wscale
    double wscale, inv_n;           // Gram: the factor between codes and values; 1 / N
    int64_t S, u0, nu;              // Gram: as LdArgs
    int W, hs;
    double* gram;
};

// THE Gram entry of section 18 from fl(X_jk): G_jk = ((s_j s_k) / N) (fl(X_jk) / (c_j c_k)), s = msig * scale, every operation in fp64 in
// this order.  Each product is commutative and X_jk = X_kj exactly, so G_jk and G_kj are the same bits whichever marker is named first.
__device__ __forceinline__ double ldd_g(double x, int64_t cj, int64_t ck, double sj, double sk, double inv_n) {
    return ((sj * sk) * inv_n) * (x / ((double)cj * (double)ck));
}

template <bool UNIFORM, int EDGE, int EP, bool SEGMENTED>
__global__ __launch_bounds__(256) void k_ldd_block(const LddArgs a) {
    constexpr int T = EDGE / 16;                    // 16-marker tiles per side
    constexpr int TW = EDGE / 32;                   // ... per wave and side
    constexpr int F = EDGE / 64;                    // 64-marker row groups per side
    constexpr int NPL = UNIFORM ? 1 : 2;            // planes per side: V (and P)
    constexpr int NP = UNIFORM ? 1 : 4;             // products
    constexpr int PIECES = 2 * EDGE * 8 / 256;      // 16-byte pieces per thread and K-step: the first half of them of side I
    // operand images of one K-step: [side: I, J][plane V, P][half of 64 individuals][16-marker tile][lane] x 16 bytes; the scores
    // epilogue reuses the space for a sub-block's 64 x 64 values of f(r^2)
    constexpr int OP_BYTES = 2 * NPL * 2 * T * 64 * 16, EP_BYTES = 64 * LD_PITCH * 8;
    __shared__ __attribute__((aligned(16))) char lds[EP == EP_SCORES && EP_BYTES > OP_BYTES ? EP_BYTES : OP_BYTES];
    v4i* op = reinterpret_cast<v4i*>(lds);
    const int64_t I = a.I0 + blockIdx.x, J = I + blockIdx.y;
    if (I >= a.nrge || J >= a.nrge) return;         // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int kp = tid & 7;                         // this thread's 16 individuals of a K-step: half kp >> 2, lane group kp & 3
    v4i acc[NP][TW][TW];
    int64_t tot[SEGMENTED ? NP : 1][SEGMENTED ? TW : 1][SEGMENTED ? TW : 1][4];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int i = 0; i < TW; i++)
#pragma unroll
            for (int j = 0; j < TW; j++) {
                acc[p][i][j] = v4i{0, 0, 0, 0};
                if (SEGMENTED)
#pragma unroll
                    for (int v = 0; v < 4; v++) tot[p][i][j][v] = 0;
            }
    // piece i of this thread: side i / (PIECES / 2), marker (tid >> 3) + 32 (i % (PIECES / 2)) of the side's group.  A marker past the
    // last re-reads it: its sums are never used.
    const uint8_t* src[PIECES];
    int dst[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; i++) {
        const int side = i / (PIECES / 2), row = (tid >> 3) + 32 * (i % (PIECES / 2));
        int64_t m = (side ? J : I) * EDGE + row;
        if (m >= a.M) m = a.M - 1;
        src[i] = a.rows + m * a.pitch + 16 * kp;
        dst[i] = ((side * NPL * 2 + (kp >> 2)) * T + (row >> 4)) * 64 + (row & 15) + 16 * (kp & 3);
    }
    uint4 o[PIECES], nm;
    // the pitch is a multiple of 64, not of 128: the second half of the last K-step may lie past the row (a piece is inside or outside
    // as a whole).  Zeros stand in; the mask bytes there are zeros too.
    auto fetch = [&](int64_t st) {
        const int64_t k0 = st * 128;
        const bool in = k0 + 16 * kp < a.pitch;
#pragma unroll
        for (int i = 0; i < PIECES; i++) o[i] = in ? *reinterpret_cast<const uint4*>(src[i] + k0) : uint4{0u, 0u, 0u, 0u};
        nm = a.nab[st * 8 + kp];
    };
    auto flush = [&]() {
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < TW; i++)
#pragma unroll
                for (int j = 0; j < TW; j++)
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        tot[SEGMENTED ? p : 0][SEGMENTED ? i : 0][SEGMENTED ? j : 0][v] += acc[p][i][j][v];
                        acc[p][i][j][v] = 0;
                    }
    };
    fetch(0);
    int64_t left = a.seg_steps;                      // K-steps until the int32 sums are flushed (SEGMENTED)
    for (int64_t st = 0; st < a.steps; st++) {
#pragma unroll
        for (int i = 0; i < PIECES; i++) {
            const bool jside = i >= PIECES / 2;
            const uint32_t ow[4] = {o[i].x, o[i].y, o[i].z, o[i].w}, mw[4] = {nm.x, nm.y, nm.z, nm.w};
            v4i V, P;
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t x = ow[d] ^ LDD_BIAS;
                if (UNIFORM) V[d] = (int)(jside ? x & mw[d] : x);
                else {
                    const uint32_t pm = jside ? ldd_present(ow[d]) & mw[d] : ldd_present(ow[d]);
                    V[d] = (int)(x & pm);
                    P[d] = (int)(pm & 0x01010101u);
                }
            }
            op[dst[i]] = V;
            if constexpr (!UNIFORM) op[dst[i] + 2 * T * 64] = P;
        }
        if (st + 1 < a.steps) fetch(st + 1);
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) {
            v4i Vi[TW], Vj[TW], Pi[UNIFORM ? 1 : TW], Pj[UNIFORM ? 1 : TW];
#pragma unroll
            for (int t = 0; t < TW; t++) {
                const int si = ((0 * NPL * 2 + h) * T + wr * TW + t) * 64 + lane, sj = ((1 * NPL * 2 + h) * T + wc * TW + t) * 64 + lane;
                Vi[t] = op[si];
                Vj[t] = op[sj];
                if constexpr (!UNIFORM) {
                    Pi[t] = op[si + 2 * T * 64];
                    Pj[t] = op[sj + 2 * T * 64];
                }
            }
#pragma unroll
            for (int i = 0; i < TW; i++)
#pragma unroll
                for (int j = 0; j < TW; j++) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Vi[i], Vj[j], acc[0][i][j], 0, 0, 0);               // VV
                    if constexpr (!UNIFORM) {
                        acc[1][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Vi[i], Pj[j], acc[1][i][j], 0, 0, 0);   // VP_ik = sum V_ni P_nk
                        acc[2][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Vj[j], acc[2][i][j], 0, 0, 0);   // VP_ki
                        acc[3][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Pj[j], acc[3][i][j], 0, 0, 0);   // PP
                    }
                }
        }
        if (SEGMENTED && --left == 0) {
            flush();
            left = a.seg_steps;
        }
        __syncthreads();
    }
    if (SEGMENTED) flush();
    // Epilogue, one 64 x 64 sub-block (Is, Js) at a time.  Register v of tile (i, j) of this lane is the entry of row
    // 16 (TW wr + i) + 4 (lane >> 4) + v, column 16 (TW wc + j) + (lane & 15) of the block: with EDGE = 128 wave 2 sa + sb holds the whole
    // sub-block (sa, sb), with EDGE = 64 the four waves share the one there is.
    double* fl = reinterpret_cast<double*>(lds);
    for (int sb = 0; sb < F * F; sb++) {
        const int64_t Is = I * F + sb / F, Js = J * F + sb % F;
        if (Js < Is || Js - Is > a.D || Js >= a.nrg) continue;       // (uniform over the workgroup; Js < Is: the mirror image holds it)
        if (F == 1 || wave == sb) {
            // (rows outside, columns inside: a row's c, T, X and chromosome are loaded once, those of the TW columns stay in registers)
#pragma unroll
            for (int i = 0; i < TW; i++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int il = (16 * (TW * wr + i) + 4 * (lane >> 4) + v) & 63;
                    const int64_t m = Is * 64 + il;
                    const bool min_ = m < a.M;
                    const int64_t cm = min_ ? a.cnt[m] : 0, tm = min_ ? a.tsum[m] : 0;
                    const double xm = min_ ? a.xd[m] : 0.0;
                    const int chi = min_ && a.chrom ? a.chrom[m] : 0;
#pragma unroll
                    for (int j = 0; j < TW; j++) {
                        const int kl = (16 * (TW * wc + j) + (lane & 15)) & 63;
                        const int64_t k = Js * 64 + kl;
                        const bool kin = k < a.M;
                        const int64_t ck = kin ? a.cnt[k] : 0, tk = kin ? a.tsum[k] : 0;
                        if constexpr (EP == EP_GRAM) {
                            // every entry of the sub-block, the diagonal included (a diagonal block holds both orders itself); a marker
                            // without a present individual keeps the zeros the Grams were cleared to
                            if (min_ && kin && cm != 0 && ck != 0) {
                                int64_t s[4];
#pragma unroll
                                for (int p = 0; p < NP; p++)
                                    s[p] = SEGMENTED ? tot[SEGMENTED ? p : 0][SEGMENTED ? i : 0][SEGMENTED ? j : 0][v] : (int64_t)acc[p][i][j][v];
                                double x;
                                if constexpr (UNIFORM) x = ldd_x(cm, ck, tm, tk, s[0], tm, tk, a.nonas);
                                else x = ldd_x(cm, ck, tm, tk, s[0], s[1], s[2], s[3]);
                                const double g = ldd_g(x, cm, ck, a.msig[m] * a.wscale, a.msig[k] * a.wscale, a.inv_n);
                                ld_gram_store(a, m, k, g, Is != Js, g);
                            }
                            continue;
                        }
                        const double xk = kin ? a.xd[k] : 0.0;
                        const int chk = kin && a.chrom ? a.chrom[k] : 0;
                        const int64_t dist = k - m;
                        const bool inband = min_ && kin && dist <= a.B && -dist <= a.B && chi == chk;
                        const bool poly = xm != 0.0 && xk != 0.0;
                        double r = 0.0;
                        if (inband && poly) {
                            if (m == k) r = 1.0;
                            else {
                                int64_t s[4];
#pragma unroll
                                for (int p = 0; p < NP; p++)
                                    s[p] = SEGMENTED ? tot[SEGMENTED ? p : 0][SEGMENTED ? i : 0][SEGMENTED ? j : 0][v] : (int64_t)acc[p][i][j][v];
                                // UNIFORM: P_j = na for every marker, so VP_jk = T_j, VP_kj = T_k and PP = nonas
                                double x;
                                if constexpr (UNIFORM) x = ldd_x(cm, ck, tm, tk, s[0], tm, tk, a.nonas);
                                else x = ldd_x(cm, ck, tm, tk, s[0], s[1], s[2], s[3]);
                                r = x / sqrt(xm * xk);
                            }
                        }
                        if (EP == EP_BAND) {
                            if (inband) {
                                const int64_t w = 2 * a.B + 1;
                                if (m >= a.j0 && m < a.j0 + a.nj) a.band[(m - a.j0) * w + a.B + dist] = r;
                                if (Is != Js && k >= a.j0 && k < a.j0 + a.nj) a.band[(k - a.j0) * w + a.B - dist] = r;     // the mirror image
                            }
                        } else {
                            fl[il * LD_PITCH + kl] = inband && poly && m != k ? ld_f(r, a.adjusted, a.nm2) : __builtin_nan("");
                        }
                    }
                }
        }
        if (EP != EP_SCORES) continue;
        __syncthreads();
        // rows of Is summed over the columns in ascending k (threads 0..63); columns of Js over the rows in ascending order (64..127)
        if (tid < 128 && (tid < 64 || Is != Js)) {
            const bool col = tid >= 64;
            const int e = tid & 63;
            double s = 0.0;
            int n = 0;
            for (int t = 0; t < 64; t++) {
                const double f = col ? fl[t * LD_PITCH + e] : fl[e * LD_PITCH + t];
                if (f == f) {
                    s += f;
                    n++;
                }
            }
            const int64_t m = (col ? Js : Is) * 64 + e;
            const int64_t slot = col ? a.D - (Js - Is) : a.D + (Js - Is);
            a.part[slot * a.Mp + m] = s;
            a.pcnt[slot * a.Mp + m] = n;
        }
        __syncthreads();
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

}  // namespace

using namespace gvi;

// what every user of k_ld_block needs resident: 2-bit genotypes in a re-encoded layout, the marker statistics and the mask words, and an
// N within the int32 invariant.  who: the caller's name; why: its reason for wanting genotypes
int gvi::planes_check(gv_ctx* c, const char* who, const char* why) {
    REFUSE_DOSAGE(c, who, why);
    if (c->dense.resident) return fail(c, "%s: refused for dense (meth) data -- %s", who, why);
    if (!c->have_stripes)
        return fail(c, "%s: needs a re-encoded genotype layout resident (tile layout or two stripe sets); raw rows alone are not supported", who);
    if (!c->have_stats || !c->mask2) return fail(c, "%s: marker statistics must be computed first", who);
    if (c->N > LD_N_MAX)
        return fail(c, "%s: N = %lld exceeds %lld, the most individuals whose products fit the int32 accumulators (4 per individual)", who,
                    (long long)c->N, (long long)LD_N_MAX);
    return 0;
}

// the window Grams of section 13: G_u of every half-grid window that overlaps the shard, W x W each and zero beyond its clipped length
void gvp::gram(hipStream_t s, const void* lay, int layout, int64_t nkb, const uint32_t* mask2, int64_t P4, int64_t N, int64_t S, int64_t M,
               int W, const double* mave, const double* msig, double* out) {
    LdArgs a{};
    a.lay = reinterpret_cast<const uint4*>(lay);
    a.nkb = nkb;
    a.mask2 = mask2;
    a.P4 = P4;
    a.N = N;
    a.M = M;
    a.nrg = (M + 63) / 64;
    a.mave = mave;
    a.msig = msig;
    a.S = S;
    a.u0 = first_window(S, W);
    a.nu = num_windows(S, M, W);
    a.W = W;
    a.hs = W == 32 ? 4 : (W == 64 ? 5 : 6);
    a.gram = out;
    if (a.nu == 0) return;
    (void)hipMemsetAsync(out, 0, sizeof(double) * (size_t)a.nu * W * W, s);      // (an error stays for the caller's hipGetLastError)
    // blocks (I, I + d) up to the most row groups that one window's markers [lo, hi) straddle
    const int64_t H = W / 2;
    int64_t D = 0;
    for (int64_t u = a.u0; u < a.u0 + a.nu; u++) {
        const int64_t lo = std::max((u - 1) * H, S) - S, hi = std::min((u + 1) * H, S + M) - S;
        D = std::max(D, (hi - 1) / 64 - lo / 64);
    }
    const dim3 grid((unsigned)a.nrg, (unsigned)(D + 1));
    if (layout == 1) hipLaunchKernelGGL((k_ld_block<1, EP_GRAM>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_ld_block<2, EP_GRAM>), grid, dim3(256), 0, s, a);
}

// what both entry points check
static int ld_check(gv_ctx* c, const char* who, int64_t window) {
    if (ld_dosage(c)) {
        if (c->dense.bits != 8)
            return fail(c, "%s: gv_set_ld_dosage covers 8-bit codes only: the resident data are 16-bit codes (their hi / lo byte split is not built)", who);
        if (!c->mask2) return fail(c, "%s: the phenotype mask must be set first (gv_set_mask)", who);
        if (c->N > LD_N_MAX)
            return fail(c, "%s: N = %lld exceeds %lld, the most individuals whose centred products fit the 128-bit integers", who, (long long)c->N,
                        (long long)LD_N_MAX);
        if (window < 1 || window > LD_WINDOW_MAX)
            return fail(c, "%s: window must be in [1, %lld] markers (%lld was passed)", who, (long long)LD_WINDOW_MAX, (long long)window);
        return 0;
    }
    if (planes_check(c, who, "LD is computed from 2-bit genotypes only")) return 1;
    if (window < 1 || window > LD_WINDOW_MAX) return fail(c, "%s: window must be in [1, %lld] markers (%lld was passed)", who, (long long)LD_WINDOW_MAX, (long long)window);
    return 0;
}

// the (j, k) entries of the band of rows [j0, j0 + nj), self included, chromosomes ignored
static double ld_entries(int64_t M, int64_t B, int64_t j0, int64_t nj) {
    double e = 0.0;
    for (int64_t j = j0; j < j0 + nj; j++) e += (double)(std::min(j + B, M - 1) - std::max(j - B, (int64_t)0) + 1);
    return e;
}

// ld_run for 8-bit dosage codes (section 17)
template <bool UNIFORM, int EDGE>
static void ldd_launch(hipStream_t s, dim3 grid, const LddArgs& a, int ep, bool seg) {
    if (ep == EP_GRAM) {        // (EDGE = 64 only: the build runs once per data set and reaches d <= 2 row groups)
        if constexpr (EDGE == 64) {
            if (seg) hipLaunchKernelGGL((k_ldd_block<UNIFORM, 64, EP_GRAM, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_ldd_block<UNIFORM, 64, EP_GRAM, false>), grid, dim3(256), 0, s, a);
        }
    } else if (ep == EP_BAND) {
        if (seg) hipLaunchKernelGGL((k_ldd_block<UNIFORM, EDGE, EP_BAND, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_ldd_block<UNIFORM, EDGE, EP_BAND, false>), grid, dim3(256), 0, s, a);
    } else {
        if (seg) hipLaunchKernelGGL((k_ldd_block<UNIFORM, EDGE, EP_SCORES, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_ldd_block<UNIFORM, EDGE, EP_SCORES, false>), grid, dim3(256), 0, s, a);
    }
}

// gram != NULL (the preconditioner's build, gvp::gram_dosage): the W x W Grams of the pc_nu half-grid windows into that DEVICE buffer
// instead -- no band, no scores, no copy to the host, gv_ld_info untouched
static int ldd_run(gv_ctx* c, const char* who, int64_t B, const int* chrom, int adjusted, double* l2, double* npairs, int64_t j0, int64_t nj,
                   double* band, double* gram = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t M = c->M, nrg = (M + 63) / 64;
    const int W = c->pc_W;
    const int64_t u0 = gvp::first_window(c->S, W), nu = gvp::num_windows(c->S, M, W);
    int D = (int)((B + 63) / 64);
    if (gram) {     // blocks (I, I + d) up to the most row groups that one window's markers [lo, hi) straddle, as gvp::gram
        D = 0;
        for (int64_t u = u0; u < u0 + nu; u++) {
            const int64_t lo = std::max((u - 1) * (W / 2), c->S) - c->S, hi = std::min((u + 1) * (W / 2), c->S + M) - c->S;
            D = std::max(D, (int)((hi - 1) / 64 - lo / 64));
        }
    }
    const bool uniform = !dosage_na_kernels(c);
    const int edge = uniform && !gram ? c->ld_dosage_edge : 64, F = edge / 64;
    Scratch w;
    LddArgs a{};
    a.rows = reinterpret_cast<const uint8_t*>(c->dense.rows);
    a.pitch = c->dense.pitch;
    a.N = c->N;
    a.M = M;
    a.B = B;
    a.nonas = c->nonas;
    // THE place that cuts the K-segments of k_ldd_block (the invariant: next to LD_N_MAX)
    a.steps = (c->N + LDD_KSTEP - 1) / LDD_KSTEP;
    a.seg_steps = std::max<int64_t>(std::min<int64_t>(c->dosage_seg, gvdm::SEG_MAX) / LDD_KSTEP, 1);
    const bool seg = a.steps > a.seg_steps;
    a.nrg = nrg;
    a.nrge = (M + edge - 1) / edge;
    a.adjusted = adjusted;
    a.nm2 = (double)c->nonas - 2.0;
    a.D = D;
    a.Mp = nrg * 64;
    a.j0 = j0;
    a.nj = nj;
    uint32_t* nab = nullptr;
    int64_t *cnt = nullptr, *tsum = nullptr, *vvd = nullptr;
    double* xd = nullptr;
    int* dchrom = nullptr;
    double *dl2 = nullptr, *dnp = nullptr;
    const size_t nband = band ? (size_t)nj * (size_t)(2 * B + 1) : 0, nslots = (size_t)(2 * D + 1);
    const int64_t nwords = std::max<int64_t>(a.steps, 1) * (LDD_KSTEP / 4);
#define LDALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)
    LDALLOC(nab, (size_t)nwords);
    LDALLOC(cnt, (size_t)M);
    LDALLOC(tsum, (size_t)M);
    LDALLOC(vvd, (size_t)M);
    LDALLOC(xd, (size_t)M);
    if (chrom) LDALLOC(dchrom, (size_t)M);
    if (gram) {
        a.msig = c->msig;
        a.wscale = c->dense.scale;
        a.inv_n = 1.0 / (double)c->N;
        a.S = c->S;
        a.u0 = u0;
        a.nu = nu;
        a.W = W;
        a.hs = W == 32 ? 4 : (W == 64 ? 5 : 6);
        a.gram = gram;
    } else if (band) LDALLOC(a.band, nband);
    else {
        LDALLOC(a.part, nslots * (size_t)a.Mp);
        LDALLOC(a.pcnt, nslots * (size_t)a.Mp);
        LDALLOC(dl2, (size_t)M);
        LDALLOC(dnp, (size_t)M);
    }
#undef LDALLOC
    a.nab = reinterpret_cast<const uint4*>(nab);
    a.cnt = cnt;
    a.tsum = tsum;
    a.xd = xd;
    a.chrom = dchrom;
    if (chrom) HIPCHK(c, hipMemcpyAsync(dchrom, chrom, sizeof(int) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    if (gram) {
        if (nu > 0) HIPCHK(c, hipMemsetAsync(gram, 0, sizeof(double) * (size_t)nu * W * W, c->stream));
    } else if (band) HIPCHK(c, hipMemsetAsync(a.band, 0, sizeof(double) * nband, c->stream));
    else {
        HIPCHK(c, hipMemsetAsync(a.part, 0, sizeof(double) * nslots * (size_t)a.Mp, c->stream));
        HIPCHK(c, hipMemsetAsync(a.pcnt, 0, sizeof(int) * nslots * (size_t)a.Mp, c->stream));
    }
    int64_t blocks = 0;
    if (M > 0 && (!band || nj > 0)) {
        hipLaunchKernelGGL(k_ldd_mask, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, c->stream, c->mask2, c->pitch / 4, c->N, nwords, nab);
        KCHK(c);
        if (uniform) hipLaunchKernelGGL(k_ldd_diag<false>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c->stream, a.rows, a.pitch, a.nab, M, cnt, tsum, vvd, xd);
        else hipLaunchKernelGGL(k_ldd_diag<true>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c->stream, a.rows, a.pitch, a.nab, M, cnt, tsum, vvd, xd);
        KCHK(c);
        // groups of `edge` markers: (I, I + d) holds the sub-blocks of 64-marker row groups at distances F d - (F - 1) .. F d + (F - 1);
        // band mode: the groups that hold a requested row, or whose blocks mirror into one
        const int64_t De = (D + F - 1) / F;
        const int64_t Ia = band ? std::max<int64_t>(j0 / 64 - D, 0) / F : 0, Ib = band ? (j0 + nj - 1) / 64 / F : a.nrge - 1;
        a.I0 = Ia;
        const dim3 grid((unsigned)(Ib - Ia + 1), (unsigned)(De + 1));
        for (int64_t I = Ia; I <= Ib; I++) blocks += (std::min<int64_t>(De, a.nrge - 1 - I) + 1) * F * F;
        const int ep = gram ? EP_GRAM : (band ? EP_BAND : EP_SCORES);
        if (!uniform) ldd_launch<false, 64>(c->stream, grid, a, ep, seg);
        else if (edge == 64) ldd_launch<true, 64>(c->stream, grid, a, ep, seg);
        else ldd_launch<true, 128>(c->stream, grid, a, ep, seg);
        KCHK(c);
        if (!band && !gram) {
            hipLaunchKernelGGL(k_ld_finish, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, a.part, a.pcnt, (int)nslots, a.Mp, M, xd,
                               dl2, dnp);
            KCHK(c);
        }
    }
    if (gram) {      // (the scratch is freed on return: the kernels that read it must have run)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    if (band) {
        if (nband) HIPCHK(c, hipMemcpyAsync(band, a.band, sizeof(double) * nband, hipMemcpyDeviceToHost, c->stream));
    } else if (M > 0) {
        HIPCHK(c, hipMemcpyAsync(l2, dl2, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
        if (npairs) HIPCHK(c, hipMemcpyAsync(npairs, dnp, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ld_last.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->ld_last.block_pairs = blocks;
    c->ld_last.useful_macs = (uniform ? 1.0 : 4.0) * (double)c->N * (band ? ld_entries(M, B, j0, nj) : ld_entries(M, B, 0, M));
    c->ld_last.scratch_bytes = (double)w.bytes;
    c->ld_last_passes = 1;
    return 0;
}

// what the Gram build of 8-bit codes needs (the dosage side of planes_check): gv_set_ld_dosage on, 8-bit codes, the mask, the marker
// statistics (unlike the LD calls: msig enters the Grams) and an N within the 128-bit epilogue
int gvi::gram_dosage_check(gv_ctx* c, const char* who) {
    // (the option was switched off after kind 1 was accepted, or codes replaced a bed under kind 1: never the bed kernel on dosage rows)
    if (!ld_dosage(c)) REFUSE_DOSAGE(c, who, "genotype windows only, unless gv_set_ld_dosage(ctx, 1) is in force (it is off)");
    if (!ld_dosage(c)) return fail(c, "%s: no compact dosage data resident", who);
    if (c->dense.bits != 8)
        return fail(c, "%s: gv_set_ld_dosage covers 8-bit codes only: the resident data are 16-bit codes (their hi / lo byte split is not built)", who);
    if (!c->mask2) return fail(c, "%s: the phenotype mask must be set first (gv_set_mask)", who);
    if (!c->have_stats) return fail(c, "%s: marker statistics must be computed first", who);
    if (c->N > LD_N_MAX)
        return fail(c, "%s: N = %lld exceeds %lld, the most individuals whose centred products fit the 128-bit integers", who, (long long)c->N,
                    (long long)LD_N_MAX);
    return 0;
}

// the window Grams of section 18 into out (device, pc_nu x W x W, W = pc_W): zeroed, then the Gram epilogue of k_ldd_block
int gvp::gram_dosage(gv_ctx* c, double* out) {
    return ldd_run(c, "LD preconditioner", 0, nullptr, 0, nullptr, nullptr, 0, c->M, nullptr, out);
}

// scores (band == NULL) or the band rows [j0, j0 + nj)
static int ld_run(gv_ctx* c, const char* who, int64_t B, const int* chrom, int adjusted, double* l2, double* npairs, int64_t j0, int64_t nj,
                  double* band) {
    if (ld_dosage(c)) return ldd_run(c, who, B, chrom, adjusted, l2, npairs, j0, nj, band);
    const auto t0 = std::chrono::steady_clock::now();
    const gvm::Plan& pl = c->plan;
    const int64_t M = c->M, nrg = (M + 63) / 64;
    const int D = (int)((B + 63) / 64);
    Scratch w;
    LdArgs a{};
    a.lay = reinterpret_cast<const uint4*>(pl.layout == 1 ? pl.tiles : pl.stripes_m);
    a.nkb = pl.nkb_m;
    a.mask2 = c->mask2;
    a.P4 = c->pitch / 4;
    a.N = c->N;
    a.M = M;
    a.B = B;
    a.nrg = nrg;
    a.mave = c->mave;
    a.msig = c->msig;
    a.adjusted = adjusted;
    a.nm2 = (double)c->nonas - 2.0;
    a.D = D;
    a.Mp = nrg * 64;
    a.j0 = j0;
    a.nj = nj;
    double* cdiag = nullptr;
    int* dchrom = nullptr;
    double *dl2 = nullptr, *dnp = nullptr;
    const size_t nband = band ? (size_t)nj * (size_t)(2 * B + 1) : 0, nslots = (size_t)(2 * D + 1);
#define LDALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)
    LDALLOC(cdiag, (size_t)M);
    if (chrom) LDALLOC(dchrom, (size_t)M);
    if (band) LDALLOC(a.band, nband);
    else {
        LDALLOC(a.part, nslots * (size_t)a.Mp);
        LDALLOC(a.pcnt, nslots * (size_t)a.Mp);
        LDALLOC(dl2, (size_t)M);
        LDALLOC(dnp, (size_t)M);
    }
#undef LDALLOC
    a.cdiag = cdiag;
    a.chrom = dchrom;
    if (chrom) HIPCHK(c, hipMemcpyAsync(dchrom, chrom, sizeof(int) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    if (band) HIPCHK(c, hipMemsetAsync(a.band, 0, sizeof(double) * nband, c->stream));
    else {
        HIPCHK(c, hipMemsetAsync(a.part, 0, sizeof(double) * nslots * (size_t)a.Mp, c->stream));
        HIPCHK(c, hipMemsetAsync(a.pcnt, 0, sizeof(int) * nslots * (size_t)a.Mp, c->stream));
    }
    int64_t blocks = 0;
    if (M > 0 && (!band || nj > 0)) {
        if (pl.layout == 1)
            hipLaunchKernelGGL(k_ld_diag<1>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
        else
            hipLaunchKernelGGL(k_ld_diag<2>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
        KCHK(c);
        // band mode: the row groups I that hold a requested row, or whose blocks (I, I + d) mirror into one
        const int64_t Ia = band ? std::max<int64_t>(j0 / 64 - D, 0) : 0, Ib = band ? (j0 + nj - 1) / 64 : nrg - 1;
        a.I0 = Ia;
        const dim3 grid((unsigned)(Ib - Ia + 1), (unsigned)(D + 1));
        for (int64_t I = Ia; I <= Ib; I++) blocks += std::min<int64_t>(D, nrg - 1 - I) + 1;
        if (band) {
            if (pl.layout == 1) hipLaunchKernelGGL((k_ld_block<1, EP_BAND>), grid, dim3(256), 0, c->stream, a);
            else hipLaunchKernelGGL((k_ld_block<2, EP_BAND>), grid, dim3(256), 0, c->stream, a);
        } else {
            if (pl.layout == 1) hipLaunchKernelGGL((k_ld_block<1, EP_SCORES>), grid, dim3(256), 0, c->stream, a);
            else hipLaunchKernelGGL((k_ld_block<2, EP_SCORES>), grid, dim3(256), 0, c->stream, a);
        }
        KCHK(c);
        if (!band) {
            hipLaunchKernelGGL(k_ld_finish, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, a.part, a.pcnt, (int)nslots, a.Mp, M,
                               cdiag, dl2, dnp);
            KCHK(c);
        }
    }
    if (band) {
        if (nband) HIPCHK(c, hipMemcpyAsync(band, a.band, sizeof(double) * nband, hipMemcpyDeviceToHost, c->stream));
    } else if (M > 0) {
        HIPCHK(c, hipMemcpyAsync(l2, dl2, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
        if (npairs) HIPCHK(c, hipMemcpyAsync(npairs, dnp, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ld_last.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->ld_last.block_pairs = blocks;
    c->ld_last.useful_macs = 4.0 * (double)c->N * (band ? ld_entries(M, B, j0, nj) : ld_entries(M, B, 0, M));
    c->ld_last.scratch_bytes = (double)w.bytes;
    c->ld_last_passes = 1;
    return 0;
}

// gv_ld_scores_pos (section 19): the band of every marker from its position, scores per annotation category.  The block kernel's EP_POS
// epilogue over the list of the blocks that hold an in-band pair, in as many passes over consecutive row groups as keep the partials within c->ld_part_bytes.
static int ld_pos_run(gv_ctx* c, const char* who, const gvw::Window& win, int adjusted, const double* annot, int C, double* l2, double* npairs) {
    const auto t0 = std::chrono::steady_clock::now();
    const gvm::Plan& pl = c->plan;
    const int64_t M = c->M, nrg = (M + 63) / 64;
    const int dmax = (int)win.dmax;
    // one row group's worth of slots: 2 dmax + 1 blocks x 64 markers x (C sums and a count)
    const double per_rg = (double)(2 * dmax + 1) * 64.0 * (8.0 * C + 4.0);
    if (per_rg > c->ld_part_bytes)
        return fail(c, "%s: the budget of the partial sums, %.0f bytes (GV_LD_PART_MB), cannot hold one row group's worth of slots: (2 * %d + 1) blocks "
                       "x 64 markers x (8 * %d + 4) bytes = %.0f bytes", who, c->ld_part_bytes, dmax, C, per_rg);
    const int64_t rgp = std::max<int64_t>(std::min<int64_t>(nrg, (int64_t)(c->ld_part_bytes / per_rg)), 1);      // row groups per pass
    const int64_t passes = (nrg + rgp - 1) / rgp;
    Scratch w;
    LdArgs a{};
    a.lay = reinterpret_cast<const uint4*>(pl.layout == 1 ? pl.tiles : pl.stripes_m);
    a.nkb = pl.nkb_m;
    a.mask2 = c->mask2;
    a.P4 = c->pitch / 4;
    a.N = c->N;
    a.M = M;
    a.nrg = nrg;
    a.mave = c->mave;
    a.msig = c->msig;
    a.adjusted = adjusted;
    a.nm2 = (double)c->nonas - 2.0;
    a.ncat = C;
    a.dmax = dmax;
    double *cdiag = nullptr, *dannot = nullptr, *dl2 = nullptr, *dnp = nullptr;
    int64_t* dhi = nullptr;
    int* dpairs = nullptr;
    std::vector<std::vector<int>> lists;       // (the host side of an asynchronous copy: alive until the call's synchronise)
    const size_t nrow = (size_t)rgp * (size_t)(dmax + 1) * 64, ncol = (size_t)rgp * (size_t)dmax * 64;
#define LDALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)
    LDALLOC(cdiag, (size_t)M);
    LDALLOC(dhi, (size_t)M);
    if (annot) LDALLOC(dannot, (size_t)M * (size_t)C);
    LDALLOC(a.part, nrow * (size_t)C);
    LDALLOC(a.pcnt, nrow);
    LDALLOC(a.cpart, ncol * (size_t)C);
    LDALLOC(a.ccnt, ncol);
    LDALLOC(dl2, (size_t)M * (size_t)C);
    LDALLOC(dnp, (size_t)M);
    LDALLOC(dpairs, 2 * (size_t)rgp * (size_t)(dmax + 1));
#undef LDALLOC
    a.cdiag = cdiag;
    a.hi = dhi;
    a.pairs = dpairs;
    a.annot = dannot;
    HIPCHK(c, hipMemcpyAsync(dhi, win.hi.data(), sizeof(int64_t) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    if (annot) HIPCHK(c, hipMemcpyAsync(dannot, annot, sizeof(double) * (size_t)M * (size_t)C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dl2, 0, sizeof(double) * (size_t)M * (size_t)C, c->stream));
    HIPCHK(c, hipMemsetAsync(dnp, 0, sizeof(double) * (size_t)M, c->stream));
    if (pl.layout == 1)
        hipLaunchKernelGGL(k_ld_diag<1>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
    else
        hipLaunchKernelGGL(k_ld_diag<2>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
    KCHK(c);
    int64_t blocks = 0;
    for (int64_t I = 0; I < nrg; I++) blocks += win.hi[(size_t)std::min(I * 64 + 63, M - 1)] / 64 - I + 1;
    for (int64_t Ia = 0; Ia < nrg; Ia += rgp) {
        const int64_t Ib = std::min(Ia + rgp, nrg) - 1;
        // (the slots of the blocks that are not launched read as zero)
        HIPCHK(c, hipMemsetAsync(a.part, 0, sizeof(double) * nrow * (size_t)C, c->stream));
        HIPCHK(c, hipMemsetAsync(a.pcnt, 0, sizeof(int) * nrow, c->stream));
        if (ncol) {
            HIPCHK(c, hipMemsetAsync(a.cpart, 0, sizeof(double) * ncol * (size_t)C, c->stream));
            HIPCHK(c, hipMemsetAsync(a.ccnt, 0, sizeof(int) * ncol, c->stream));
        }
        a.I0 = Ia;
        // the blocks (I, I + d) that hold an in-band pair -- hi does not decrease, so the last marker of I reaches furthest -- with d
        // outermost, the order in which the index window's grid (row groups, D + 1) dispatches its blocks
        lists.emplace_back();
        std::vector<int>& L = lists.back();
        for (int d = 0; d <= dmax; d++)
            for (int64_t I = Ia; I <= Ib; I++)
                if (win.hi[(size_t)std::min(I * 64 + 63, M - 1)] / 64 - I >= d) {
                    L.push_back((int)I);
                    L.push_back((int)(I + d));
                }
        HIPCHK(c, hipMemcpyAsync(dpairs, L.data(), sizeof(int) * L.size(), hipMemcpyHostToDevice, c->stream));
        const dim3 grid((unsigned)(L.size() / 2));
        if (pl.layout == 1) hipLaunchKernelGGL((k_ld_block<1, EP_POS>), grid, dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL((k_ld_block<2, EP_POS>), grid, dim3(256), 0, c->stream, a);
        KCHK(c);
        const int64_t span = (std::min<int64_t>(Ib + dmax, nrg - 1) - Ia + 1) * 64 * C;
        hipLaunchKernelGGL(k_ld_finish_pos, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, c->stream, a.part, a.pcnt, a.cpart, a.ccnt, dmax, C, Ia,
                           Ib, nrg, M, cdiag, dannot, dl2, dnp);
        KCHK(c);
    }
    HIPCHK(c, hipMemcpyAsync(l2, dl2, sizeof(double) * (size_t)M * (size_t)C, hipMemcpyDeviceToHost, c->stream));
    if (npairs) HIPCHK(c, hipMemcpyAsync(npairs, dnp, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ld_last.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->ld_last.block_pairs = blocks;
    c->ld_last.useful_macs = 4.0 * (double)c->N * win.entries;
    c->ld_last.scratch_bytes = (double)w.bytes;
    c->ld_last_passes = (int)passes;
    return 0;
}

// gv_ld_clump (section 20): the EP_ADJ epilogue over the filtered list of blocks, then the selection in rounds of k_clump_round, then
// k_clump_assign.  index_of: M host int64.
static int ld_clump_run(gv_ctx* c, const char* who, const gvw::Window& win, const gvc::Plan& cp, double r2, int64_t* index_of) {
    const auto t0 = std::chrono::steady_clock::now();
    const gvm::Plan& pl = c->plan;
    const int64_t M = c->M, nrg = (M + 63) / 64;
    const int dmax = (int)win.dmax;
    constexpr int BATCH = 16;        // rounds between two reads of the undecided counters
    Scratch w;
    LdArgs a{};
    a.lay = reinterpret_cast<const uint4*>(pl.layout == 1 ? pl.tiles : pl.stripes_m);
    a.nkb = pl.nkb_m;
    a.mask2 = c->mask2;
    a.P4 = c->pitch / 4;
    a.N = c->N;
    a.M = M;
    a.nrg = nrg;
    a.mave = c->mave;
    a.msig = c->msig;
    a.dmax = dmax;
    a.r2 = r2;
    double* cdiag = nullptr;
    int64_t *dhi = nullptr, *dindex = nullptr;
    int *dpairs = nullptr, *drank = nullptr, *dorder = nullptr, *dstate = nullptr, *dleft = nullptr;
    const size_t nwords = (size_t)nrg * (size_t)(2 * dmax + 1) * 64;
#define LDALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)
    LDALLOC(cdiag, (size_t)M);
    LDALLOC(dhi, (size_t)M);
    LDALLOC(drank, (size_t)M);
    LDALLOC(dorder, (size_t)cp.n_e1);
    LDALLOC(dstate, (size_t)M);
    LDALLOC(dleft, (size_t)BATCH);
    LDALLOC(dindex, (size_t)M);
    LDALLOC(dpairs, cp.pairs.size());
    LDALLOC(a.adjw, nwords);
#undef LDALLOC
    a.cdiag = cdiag;
    a.hi = dhi;
    a.pairs = dpairs;
    a.crank = drank;
    HIPCHK(c, hipMemcpyAsync(dhi, win.hi.data(), sizeof(int64_t) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(drank, cp.rank.data(), sizeof(int) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    if (cp.n_e1) HIPCHK(c, hipMemcpyAsync(dorder, cp.order.data(), sizeof(int) * (size_t)cp.n_e1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dstate, 0, sizeof(int) * (size_t)M, c->stream));
    // (the words of the blocks that are not launched read as no edge)
    HIPCHK(c, hipMemsetAsync(a.adjw, 0, sizeof(uint64_t) * nwords, c->stream));
    const int64_t blocks = (int64_t)(cp.pairs.size() / 2);
    if (blocks) {
        if (pl.layout == 1)
            hipLaunchKernelGGL(k_ld_diag<1>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
        else
            hipLaunchKernelGGL(k_ld_diag<2>, dim3((unsigned)nrg), dim3(256), 0, c->stream, a.lay, a.nkb, a.mask2, a.P4, a.N, M, a.mave, a.msig, cdiag);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(dpairs, cp.pairs.data(), sizeof(int) * cp.pairs.size(), hipMemcpyHostToDevice, c->stream));
        if (pl.layout == 1) hipLaunchKernelGGL((k_ld_block<1, EP_ADJ>), dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL((k_ld_block<2, EP_ADJ>), dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
        KCHK(c);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const auto t1 = std::chrono::steady_clock::now();
    // the rounds: the undecided marker of the lowest rank is decided in every round, so |E1| rounds decide them all
    int64_t rounds = 0;
    int left[BATCH] = {0};
    bool open = cp.n_e1 > 0;
    while (open) {
        if (rounds > cp.n_e1)
            return fail(c, "%s: the selection has not finished after %lld rounds over %lld index candidates (%d still undecided): this cannot "
                           "happen", who, (long long)rounds, (long long)cp.n_e1, left[BATCH - 1]);
        HIPCHK(c, hipMemsetAsync(dleft, 0, sizeof(int) * BATCH, c->stream));
        for (int b = 0; b < BATCH; b++) {
            hipLaunchKernelGGL(k_clump_round, dim3((unsigned)((cp.n_e1 + 255) / 256)), dim3(256), 0, c->stream, a.adjw, dorder, drank, cp.n_e1, dmax, nrg,
                               dstate, dleft + b);
            KCHK(c);
        }
        HIPCHK(c, hipMemcpyAsync(left, dleft, sizeof(int) * BATCH, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < BATCH && open; b++) {
            rounds++;
            open = left[b] != 0;
        }
    }
    hipLaunchKernelGGL(k_clump_assign, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, a.adjw, drank, dstate, dmax, nrg, M, dindex);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(index_of, dindex, sizeof(int64_t) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const auto t2 = std::chrono::steady_clock::now();
    c->ld_last.seconds = std::chrono::duration<double>(t2 - t0).count();
    c->ld_last.block_pairs = blocks;
    c->ld_last.useful_macs = 4.0 * (double)c->N * cp.pairs_e2;
    c->ld_last.scratch_bytes = (double)w.bytes;
    c->ld_last_passes = 1;
    c->clump_rounds = (int)rounds;
    c->clump_n_e1 = cp.n_e1;
    c->clump_n_e2 = cp.n_e2;
    c->clump_block_s = std::chrono::duration<double>(t1 - t0).count();
    c->clump_select_s = std::chrono::duration<double>(t2 - t1).count();
    return 0;
}

// the refusals of a positional window (gv_ld_scores_pos, gv_ld_clump)
static int ld_window_check(gv_ctx* c, const char* who, const gvw::Window& win, const double* pos, const int* chrom) {
    const long long at = (long long)win.at;
    switch (win.verdict) {
        case gvw::OK: break;
        case gvw::POS_NOT_FINITE: return fail(c, "%s: pos[%lld] is not finite", who, at);
        case gvw::POS_DECREASES:
            return fail(c, "%s: pos[%lld] = %.17g is below pos[%lld] = %.17g on the same chromosome: positions must not decrease", who, at, pos[at],
                        at - 1, pos[at - 1]);
        case gvw::CHROM_REAPPEARS:
            return fail(c, "%s: chromosome id %d reappears at marker %lld after its run has ended: every chromosome must be one contiguous run", who,
                        chrom[at], at);
        case gvw::REACH_TOO_LONG:
            return fail(c, "%s: marker %lld reaches %lld markers ahead, more than the %lld a band may (a smaller radius, or gv_ld_scores)", who, at,
                        (long long)win.reach, (long long)LD_WINDOW_MAX);
    }
    return 0;
}

extern "C" {

int gv_ld_clump(gv_ctx* c, const double* pos, double radius, const int* chrom, const double* p, double p1, double p2, double r2,
                int64_t* index_of, int64_t* n_index) {
    const char* who = "gv_ld_clump";
    if (c->dense.resident && c->dense.bits)
        return fail(c, "%s: bed data only for now: compact dosage data (%d-bit codes) are not served by this entry point, with or without "
                       "gv_set_ld_dosage", who, c->dense.bits);
    if (planes_check(c, who, "LD is computed from 2-bit genotypes only")) return 1;
    NEED(c, pos, "gv_ld_clump: pos is NULL");
    NEED(c, p, "gv_ld_clump: p is NULL");
    NEED(c, index_of, "gv_ld_clump: index_of is NULL");
    if (!std::isfinite(radius) || radius < 0.0) return fail(c, "%s: radius must be finite and >= 0 (%g was passed)", who, radius);
    if (!std::isfinite(p1) || !std::isfinite(p2)) return fail(c, "%s: p1 and p2 must be finite (%g and %g were passed)", who, p1, p2);
    if (!std::isfinite(r2)) return fail(c, "%s: r2 must be finite (%g was passed)", who, r2);
    if (p1 > p2) return fail(c, "%s: p1 must not exceed p2 (%g > %g): an index marker is a member too", who, p1, p2);
    if (p1 < 0.0) return fail(c, "%s: p1 must be >= 0 (%g was passed)", who, p1);
    if (r2 < 0.0 || r2 > 1.0) return fail(c, "%s: r2 must be in [0, 1] (%g was passed)", who, r2);
    const gvw::Window win = gvw::make_window(pos, chrom, radius, c->M, LD_WINDOW_MAX);
    if (ld_window_check(c, who, win, pos, chrom)) return 1;
    if (c->M == 0) return 0;
    const gvc::Plan cp = gvc::make_plan(p, p1, p2, win.hi.data(), win.dmax, c->M);
    if (ld_clump_run(c, who, win, cp, r2, index_of)) return 1;
    if (n_index) {
        int64_t n = 0;
        for (int64_t j = 0; j < c->M; j++) n += index_of[j] == j;
        *n_index = n;
    }
    return 0;
}

int gv_ld_clump_last(const gv_ctx* c, int* rounds, int64_t* n_e1, int64_t* n_e2) {
    if (rounds) *rounds = c->clump_rounds;
    if (n_e1) *n_e1 = c->clump_n_e1;
    if (n_e2) *n_e2 = c->clump_n_e2;
    return 0;
}

int gv_ld_clump_seconds(const gv_ctx* c, double* block_pass, double* selection) {
    if (block_pass) *block_pass = c->clump_block_s;
    if (selection) *selection = c->clump_select_s;
    return 0;
}

int gv_ld_scores_pos(gv_ctx* c, const double* pos, double radius, const int* chrom, int adjusted, const double* annot, int ncat, double* l2,
                     double* npairs) {
    const char* who = "gv_ld_scores_pos";
    if (c->dense.resident && c->dense.bits)
        return fail(c, "%s: bed data only for now: compact dosage data (%d-bit codes) are not served by this entry point, with or without "
                       "gv_set_ld_dosage", who, c->dense.bits);
    if (planes_check(c, who, "LD is computed from 2-bit genotypes only")) return 1;
    NEED(c, pos, "gv_ld_scores_pos: pos is NULL");
    NEED(c, l2, "gv_ld_scores_pos: l2 is NULL");
    NEED(c, adjusted == 0 || adjusted == 1, "gv_ld_scores_pos: adjusted must be 0 or 1");
    NEED(c, adjusted == 0 || c->nonas >= 3, "gv_ld_scores_pos: the adjusted estimator r^2 - (1 - r^2) / (n - 2) needs at least 3 phenotyped individuals");
    if (!std::isfinite(radius) || radius < 0.0) return fail(c, "%s: radius must be finite and >= 0 (%g was passed)", who, radius);
    if (annot && (ncat < 1 || ncat > 512)) return fail(c, "%s: ncat must be in [1, 512] when annot is given (%d was passed)", who, ncat);
    const gvw::Window win = gvw::make_window(pos, chrom, radius, c->M, LD_WINDOW_MAX);
    if (ld_window_check(c, who, win, pos, chrom)) return 1;
    if (c->M == 0) {
        c->ld_last = gv_ld_stats{};
        c->ld_last_passes = 0;
        return 0;
    }
    return ld_pos_run(c, who, win, adjusted, annot, annot ? ncat : 1, l2, npairs);
}

int gv_ld_last_passes(const gv_ctx* c, int* passes) {
    if (passes) *passes = c->ld_last_passes;
    return 0;
}

int gv_ld_scores(gv_ctx* c, int64_t window, const int* chrom, int adjusted, double* l2, double* npairs) {
    if (ld_check(c, "gv_ld_scores", window)) return 1;
    NEED(c, l2, "gv_ld_scores: l2 is NULL");
    NEED(c, adjusted == 0 || adjusted == 1, "gv_ld_scores: adjusted must be 0 or 1");
    NEED(c, adjusted == 0 || c->nonas >= 3, "gv_ld_scores: the adjusted estimator r^2 - (1 - r^2) / (n - 2) needs at least 3 phenotyped individuals");
    return ld_run(c, "gv_ld_scores", window, chrom, adjusted, l2, npairs, 0, c->M, nullptr);
}

int gv_ld_band(gv_ctx* c, int64_t window, const int* chrom, int64_t j0, int64_t nj, double* r) {
    if (ld_check(c, "gv_ld_band", window)) return 1;
    NEED(c, r, "gv_ld_band: r is NULL");
    if (j0 < 0 || nj < 0 || j0 > c->M || nj > c->M - j0)
        return fail(c, "gv_ld_band: rows [%lld, %lld) are outside the shard's markers [0, %lld)", (long long)j0, (long long)(j0 + nj), (long long)c->M);
    return ld_run(c, "gv_ld_band", window, chrom, 0, nullptr, nullptr, j0, nj, r);
}

int gv_set_ld_dosage(gv_ctx* c, int on) {
    NEED(c, on == 0 || on == 1, "gv_set_ld_dosage: on must be 0 or 1");
    if (on != c->ld_dosage) pc_invalidate(c, false);      // (the Grams of dosage codes belong to the option)
    c->ld_dosage = on;
    return 0;
}

int gv_get_ld_dosage(const gv_ctx* c, int* on) {
    if (on) *on = c->ld_dosage;
    return 0;
}

int gv_ld_info(gv_ctx* c, gv_ld_stats* info) {
    NEED(c, info, "gv_ld_info: info is NULL");
    *info = c->ld_last;
    return 0;
}

}  // extern "C"
