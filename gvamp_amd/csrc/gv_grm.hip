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
};

enum { EP_RECT, EP_PAIRS };

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
    __shared__ GrmStage stage[2];
    // Workgroups are dealt to the eight XCDs round-robin by block index: XCD x takes a contiguous eighth of the block list, so the
    // workgroups that run side by side on one L2 share their I side (gv_king.hip)
    int64_t b;
    {
        const int64_t q = a.nblocks / 8, r = a.nblocks % 8, x = blockIdx.x % 8, k = blockIdx.x / 8;
        b = x * q + (x < r ? x : r) + k;
    }
    int64_t I, J;
    if constexpr (EP == EP_RECT) {
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

int gv_grm_info(gv_ctx* c, gv_grm_stats* info) {
    if (!c || !info) return 1;
    *info = c->grm_last;
    return 0;
}

}  // extern "C"
