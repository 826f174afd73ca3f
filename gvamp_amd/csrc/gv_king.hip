// gv_king.hip -- pairwise kinship (KING-robust) of the resident 2-bit genotypes (gv_king_block, gv_king_pairs):
// the one product of the tree that is an N x N block summed over the MARKERS.
//
// With a in {0, 1, 2} the allele count the tile layout stores as r' = a (r' = 3: missing) the planes of an individual are
//   P = present,  H = [a = 1] P,  D = (a - 1) P in {-1, 0, 1},
// each multiplied by the marker selection use[m].  Five exact v_mfma_i32_16x16x64_i8 sums over the used markers per pair (i, j):
//   nsnp = P_i P_j,  hethet = H_i H_j,  het_i = H_i P_j,  het_j = P_i H_j,  dd = D_i D_j
// and one short fixed fp64 expression (king_kin below, the contract of gvamp.h).
//   k_king_mask   the K-side mask of every quad of four markers as the selector bits the decode ORs in: m < M && use[m]
//   k_king_block  one workgroup of 256 threads per pair of 64-individual groups (I <= J); the K loop runs over the shard's 64-marker row
//                 groups, two per step.  In the tile layout the 64 individuals of group I at row group rg are the 64 contiguous 16-byte
//                 pieces s * 64 ... s * 64 + 63 of super-block (rg, kb), kb = I / 4, s = I % 4: 1 KiB per side and row group.  Every thread
//                 expands what it loaded ONCE into the three i8 planes in MFMA operand order in LDS; each of the 4 waves multiplies a
//                 32 x 32 quarter (4 tiles x 5 products = 80 accumulator registers).  Epilogues: the dense rectangle (EP_RECT, over a
//                 host-built list of the blocks that touch it) or the pairs at or above a cutoff (EP_PAIRS, over the whole upper
//                 triangle by a linear block index).
// Integer sums, then the same fp64 operations for (i, j) and (j, i): the results do not depend on the kernel mode or the launch.  The
// pairs are appended through one atomic counter and sorted by (i, j) on the host, so what is delivered is a function of the data alone.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "gv_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// THE int32 invariant of this file: one marker adds at most 1 in magnitude to any of the five sums, so a sum over all markers of the
// shard stays within int32 for M <= 2^31 - 1 and no accumulation is cut into segments.  A larger shard is refused (king_check).
constexpr int64_t KING_M_MAX = 2147483647LL;
constexpr int64_t KING_BLOCKS_MAX = 2147483647LL;      // workgroups of one launch (a 1-D grid)

// The planes as byte look-ups: v_perm_b32 with the selector byte c = r' (| 4 where the marker is not used) picks byte c of
// {0, LUT}: bytes 0..3 of the look-up word answer r' = 0, 1, 2, 3; bytes 4..7 (the other source, zero) answer an unused marker.
constexpr uint32_t LUT_P = 0x00010101u;     // present: r' != 3
constexpr uint32_t LUT_H = 0x00000100u;     // heterozygous: r' == 1
constexpr uint32_t LUT_D = 0x000100FFu;     // a - 1: -1, 0, 1 (0 at missing)
constexpr uint32_t SEL_UNUSED = 0x04040404u;

// kmq[q] for quad q (markers 4 q + t, t = 0..3) of the nrg * 16 quads: byte t = 4 if the marker is past M or not selected, else 0
__global__ __launch_bounds__(256) void k_king_mask(const uint8_t* __restrict__ use, int64_t M, int64_t nq, uint32_t* __restrict__ kmq) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    uint32_t w = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int64_t m = 4 * q + t;
        const bool on = m < M && (!use || use[m] != 0);
        w |= on ? 0u : (4u << (8 * t));
    }
    kmq[q] = w;
}

// THE fp64 expression of the contract: two operations, one correctly rounded division and one subtraction; NaN without a heterozygote.
// ibs0 = (homhom - dd) / 2 is exact: homhom - dd counts every opposite-homozygote marker twice and nothing else.
__device__ __forceinline__ double king_kin(int nsnp, int hethet, int het_i, int het_j, int dd, int& ibs0) {
    const int64_t homhom = (int64_t)nsnp - het_i - het_j + hethet;
    const int64_t i0 = (homhom - dd) / 2;
    ibs0 = (int)i0;
    const int64_t d2 = 4 * i0 + ((int64_t)het_i - hethet) + ((int64_t)het_j - hethet);
    const int64_t mn = het_i < het_j ? het_i : het_j;
    if (mn == 0) return __builtin_nan("");
    const double q = (double)d2 / (double)(4 * mn);
    return 0.5 - q;
}

struct KingArgs {
    const uint32_t* tiles;          // the tile layout as dwords
    int64_t nkb, nrg;               // 256-individual blocks per row group; 64-marker row groups
    const uint32_t* kmq;            // nrg * 16 selector masks (k_king_mask)
    int64_t N, nG;                  // individuals; groups of 64 of them
    int64_t nblocks;                // blocks of the launch
    const int* blocks;              // EP_RECT: (I, J) of block b, I <= J; EP_PAIRS: NULL, the upper triangle by linear index
    int64_t i0, ni, j0, nj;         // EP_RECT: the rectangle
    double* kin;                    // EP_RECT: ni x nj or NULL
    int* counts;                    // EP_RECT: ni x nj x 5 or NULL
    double cutoff;                  // EP_PAIRS
    unsigned long long cap;         // EP_PAIRS: slots of the four arrays below
    unsigned long long* found;      // EP_PAIRS: pairs at or above the cutoff (one counter, zeroed before the launch)
    int *pi, *pj;
    double* pkin;
    int* pcounts;
};

enum { EP_RECT, EP_PAIRS };

// block b of the upper triangle of nG x nG in row-major order: row I holds J = I .. nG - 1 and starts at I nG - I (I - 1) / 2.  The fp64
// estimate of the root is corrected in exact integers.
__device__ __forceinline__ void king_block_of(int64_t b, int64_t nG, int64_t& I, int64_t& J) {
    const double t = 2.0 * (double)nG + 1.0;
    int64_t i = (int64_t)((t - sqrt(t * t - 8.0 * (double)b)) * 0.5);
    i = i < 0 ? 0 : (i > nG - 1 ? nG - 1 : i);
    while (i > 0 && i * nG - i * (i - 1) / 2 > b) i--;
    while (i + 1 < nG && (i + 1) * nG - (i + 1) * i / 2 <= b) i++;
    I = i;
    J = i + (b - (i * nG - i * (i - 1) / 2));
}

template <int EP>
__global__ __launch_bounds__(256, 2) void k_king_block(const KingArgs a) {
    // operand images of one step: [row group of the step 0, 1][side I, J][16-individual tile][plane P, H, D][lane] x 16 bytes = 48 KiB
    __shared__ v4i op[2 * 2 * 4 * 3 * 64];
    // Workgroups are dealt to the eight XCDs round-robin by block index: XCD x takes a contiguous eighth of the block list, so the
    // workgroups that run side by side on one L2 share their I side
    int64_t b;
    {
        const int64_t q = a.nblocks / 8, r = a.nblocks % 8, x = blockIdx.x % 8, k = blockIdx.x / 8;
        b = x * q + (x < r ? x : r) + k;
    }
    int64_t I, J;
    if constexpr (EP == EP_RECT) {
        I = a.blocks[2 * b];
        J = a.blocks[2 * b + 1];
    } else king_block_of(b, a.nG, I, J);
    if (I < 0 || J >= a.nG || I > J) return;        // (uniform over the workgroup; never true for a list built by the host)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    // loader coordinates: wave = (side, row group of the step); the thread takes dword d of the pieces (quad 4 g + e, jj), e = 0..3:
    // the 16 markers 16 g + [0, 16) of the individuals 16 jj + 4 d + [0, 4) of its side's group
    const int side = tid >> 7, ks = (tid >> 6) & 1, jj = lane >> 4, g = (lane >> 2) & 3, d = lane & 3;
    const int64_t G = side ? J : I;
    const int64_t rgstride = a.nkb * 1024;          // dwords per row group
    const uint32_t* src = a.tiles + ((G >> 2) * 256 + (G & 3) * 64) * 4 + 64 * g + 4 * jj + d;
    v4i acc[5][2][2];
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[p][i][j] = v4i{0, 0, 0, 0};
    const int64_t steps = (a.nrg + 1) / 2;
    uint32_t dw[4], km[4];
    auto fetch = [&](int64_t st) {
        const int64_t rg = 2 * st + ks;
        if (rg < a.nrg) {
            const uint32_t* p = src + rg * rgstride;
#pragma unroll
            for (int e = 0; e < 4; e++) dw[e] = p[16 * e];
            const uint4 m = *reinterpret_cast<const uint4*>(a.kmq + rg * 16 + 4 * g);
            km[0] = m.x;
            km[1] = m.y;
            km[2] = m.z;
            km[3] = m.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                dw[e] = 0u;
                km[e] = SEL_UNUSED;
            }
        }
    };
    if (steps > 0) fetch(0);
    for (int64_t st = 0; st < steps; st++) {
        // expand once, for the whole workgroup: field f of dword d is individual 4 d + f of the tile, its bytes four consecutive markers.
        // Lane 16 g + 4 d + f of the operand holds the 16 markers of g in K order.  The threads walk f rotated by g, so that the 16
        // threads of a tile write 16 different lanes at a time.
        v4i* dst = op + (((ks * 2 + side) * 4 + jj) * 3) * 64 + 16 * g + 4 * d;
#pragma unroll
        for (int fs = 0; fs < 4; fs++) {
            const int f = (fs + g) & 3;
            v4i P, H, D;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t sel = ((dw[e] >> (2 * f)) & 0x03030303u) | km[e];
                P[e] = (int)__builtin_amdgcn_perm(0u, LUT_P, sel);
                H[e] = (int)__builtin_amdgcn_perm(0u, LUT_H, sel);
                D[e] = (int)__builtin_amdgcn_perm(0u, LUT_D, sel);
            }
            dst[f] = P;
            dst[64 + f] = H;
            dst[128 + f] = D;
        }
        if (st + 1 < steps) fetch(st + 1);
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < 2; k2++) {
            v4i Pi[2], Hi[2], Di[2], Pj[2], Hj[2], Dj[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int si = (((k2 * 2 + 0) * 4 + 2 * wr + t) * 3) * 64 + lane, sj = (((k2 * 2 + 1) * 4 + 2 * wc + t) * 3) * 64 + lane;
                Pi[t] = op[si];
                Hi[t] = op[si + 64];
                Di[t] = op[si + 128];
                Pj[t] = op[sj];
                Hj[t] = op[sj + 64];
                Dj[t] = op[sj + 128];
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Pj[j], acc[0][i][j], 0, 0, 0);   // nsnp
                    acc[1][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Hi[i], Hj[j], acc[1][i][j], 0, 0, 0);   // hethet
                    acc[2][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Hi[i], Pj[j], acc[2][i][j], 0, 0, 0);   // het of the row individual
                    acc[3][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Pi[i], Hj[j], acc[3][i][j], 0, 0, 0);   // het of the column individual
                    acc[4][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Di[i], Dj[j], acc[4][i][j], 0, 0, 0);   // dd
                }
        }
        __syncthreads();
    }
    // Epilogue.  Register v of tile (i, j) of this lane is the pair of individual 16 (2 wr + i) + 4 (lane >> 4) + v of group I and
    // individual 16 (2 wc + j) + (lane & 15) of group J.  Pad individuals (>= N) are stored as present homozygotes: nothing is emitted.
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int64_t gj = J * 64 + 16 * (2 * wc + j) + (lane & 15);
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int64_t gi = I * 64 + 16 * (2 * wr + i) + 4 * (lane >> 4) + v;
                if (gi >= a.N || gj >= a.N) continue;
                const int nsnp = acc[0][i][j][v], hh = acc[1][i][j][v], hi = acc[2][i][j][v], hj = acc[3][i][j][v], dd = acc[4][i][j][v];
                int ibs0;
                // (min and the integer sums are symmetric in the two individuals: kin[i][j] and kin[j][i] are the same bits whichever
                // of them is taken as i)
                const double kin = king_kin(nsnp, hh, hi, hj, dd, ibs0);
                if constexpr (EP == EP_RECT) {
                    // entry [r][c] of the rectangle carries het_i of its row individual and het_j of its column individual; a block
                    // off the diagonal also owes the rectangle its mirror image
#pragma unroll
                    for (int mir = 0; mir < 2; mir++) {
                        if (mir && I == J) break;
                        const int64_t r = (mir ? gj : gi) - a.i0, c = (mir ? gi : gj) - a.j0;
                        if (r < 0 || r >= a.ni || c < 0 || c >= a.nj) continue;
                        const int64_t o = r * a.nj + c;
                        if (a.kin) a.kin[o] = kin;
                        if (a.counts) {
                            int* q = a.counts + 5 * o;
                            q[0] = nsnp;
                            q[1] = hh;
                            q[2] = ibs0;
                            q[3] = mir ? hj : hi;
                            q[4] = mir ? hi : hj;
                        }
                    }
                } else {
                    if (gi < gj && kin >= a.cutoff) {       // (a NaN never passes)
                        const unsigned long long slot = atomicAdd(a.found, 1ull);
                        if (slot < a.cap) {
                            a.pi[slot] = (int)gi;
                            a.pj[slot] = (int)gj;
                            a.pkin[slot] = kin;
                            int* q = a.pcounts + 5 * slot;
                            q[0] = nsnp;
                            q[1] = hh;
                            q[2] = ibs0;
                            q[3] = hi;
                            q[4] = hj;
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

}  // namespace

using namespace gvi;

// what both entry points need resident: 2-bit genotypes in the tile layout on a job of one rank, within the int32 invariant.  Neither
// the phenotype mask nor the marker statistics: relatedness is a property of the genotypes.
static int king_check(gv_ctx* c, const char* who) {
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    REFUSE_DOSAGE(c, who, "kinship is computed from 2-bit genotypes only");
    if (c->dense.resident) return fail(c, "%s: refused for dense (meth) data -- kinship is computed from 2-bit genotypes only", who);
    if (!c->have_stripes)
        return fail(c, "%s: needs the tile layout resident (gv_set_layout(ctx, .., 2)); raw rows alone are not supported", who);
    if (c->plan.layout != 1 || !c->plan.tiles)
        return fail(c, "%s: two stripe sets are resident, whose individuals are not contiguous per marker group -- upload under the tile layout "
                       "(gv_set_layout(ctx, .., 2))", who);
    if (is_multi(c))
        return fail(c, "%s: a job of more than one rank is refused: the counts are sums over the markers of ALL ranks, and the integer "
                       "all-reduce that would add them is not built", who);
    if (c->M > KING_M_MAX)
        return fail(c, "%s: M = %lld exceeds %lld, the most markers whose sums fit the int32 accumulators (1 per marker)", who, (long long)c->M,
                    (long long)KING_M_MAX);
    return 0;
}

#define KGALLOC(p, n)                                                                                                          \
    do {                                                                                                                       \
        if (w.get(&p, n) != hipSuccess) {                                                                                      \
            (void)hipGetLastError();                                                                                           \
            return fail(c, "%s: cannot allocate %zu bytes of device scratch (%zu already held by this call)", who, sizeof(*p) * (size_t)(n), w.bytes); \
        }                                                                                                                      \
    } while (0)

// the shared front of both calls: the argument block and the K-side mask; *used = the markers that count
static int king_prepare(gv_ctx* c, const char* who, const uint8_t* use, Scratch& w, KingArgs& a, int64_t* used) {
    const gvm::Plan& pl = c->plan;
    a.tiles = reinterpret_cast<const uint32_t*>(pl.tiles);
    a.nkb = pl.nkb_m;
    a.nrg = (c->M + 63) / 64;
    a.N = c->N;
    a.nG = (c->N + 63) / 64;
    uint32_t* kmq = nullptr;
    uint8_t* duse = nullptr;
    const int64_t nq = a.nrg * 16;
    KGALLOC(kmq, (size_t)nq);
    int64_t n = c->M;
    if (use) {
        KGALLOC(duse, (size_t)c->M);
        if (c->M > 0) HIPCHK(c, hipMemcpyAsync(duse, use, (size_t)c->M, hipMemcpyHostToDevice, c->stream));
        n = 0;
        for (int64_t m = 0; m < c->M; m++) n += use[m] != 0;
    }
    if (nq > 0) {
        hipLaunchKernelGGL(k_king_mask, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, c->stream, duse, c->M, nq, kmq);
        KCHK(c);
    }
    a.kmq = kmq;
    *used = n;
    return 0;
}

extern "C" {

int gv_king_block(gv_ctx* c, const uint8_t* use, int64_t i0, int64_t ni, int64_t j0, int64_t nj, double* kin, int32_t* counts) {
    if (!c) return 1;
    const char* who = "gv_king_block";
    if (king_check(c, who)) return 1;
    if (i0 < 0 || ni < 0 || i0 > c->N - ni || j0 < 0 || nj < 0 || j0 > c->N - nj)
        return fail(c, "%s: the rectangle [%lld, %lld) x [%lld, %lld) is outside [0, N = %lld)", who, (long long)i0, (long long)(i0 + ni),
                    (long long)j0, (long long)(j0 + nj), (long long)c->N);
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    KingArgs a{};
    int64_t used = 0;
    std::vector<int> blocks;
    if (ni > 0 && nj > 0 && (kin || counts)) {
        if (king_prepare(c, who, use, w, a, &used)) return 1;
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
        if (a.nblocks > KING_BLOCKS_MAX) return fail(c, "%s: the rectangle spans %lld blocks, more than one launch takes", who, (long long)a.nblocks);
        const size_t ne = (size_t)ni * (size_t)nj;
        int* dblocks = nullptr;
        KGALLOC(dblocks, blocks.size());
        if (kin) KGALLOC(a.kin, ne);
        if (counts) KGALLOC(a.counts, 5 * ne);
        a.blocks = dblocks;
        a.i0 = i0;
        a.ni = ni;
        a.j0 = j0;
        a.nj = nj;
        HIPCHK(c, hipMemcpyAsync(dblocks, blocks.data(), sizeof(int) * blocks.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_king_block<EP_RECT>, dim3((unsigned)a.nblocks), dim3(256), 0, c->stream, a);
        KCHK(c);
        if (kin) HIPCHK(c, hipMemcpyAsync(kin, a.kin, sizeof(double) * ne, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, a.counts, sizeof(int) * 5 * ne, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->king_last.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->king_last.block_pairs = a.nblocks;
    c->king_last.used_markers = used;
    c->king_last.pairs = a.nblocks ? ni * nj : 0;
    c->king_last.useful_macs = 5.0 * (double)used * (double)c->king_last.pairs;
    c->king_last.scratch_bytes = (double)w.bytes;
    return 0;
}

int gv_king_pairs(gv_ctx* c, const uint8_t* use, double cutoff, int64_t cap, int32_t* pi, int32_t* pj, double* kin, int32_t* counts,
                  int64_t* n_found) {
    if (!c) return 1;
    const char* who = "gv_king_pairs";
    if (king_check(c, who)) return 1;
    NEED(c, n_found, "gv_king_pairs: n_found is NULL");
    NEED(c, cap >= 0, "gv_king_pairs: cap must not be negative");
    NEED(c, cap == 0 || (pi && pj && kin && counts), "gv_king_pairs: pi, pj, kin or counts is NULL with cap > 0");
    if (std::isnan(cutoff) || cutoff == INFINITY) return fail(c, "gv_king_pairs: cutoff must be a finite number or -inf (every pair)");
    const auto t0 = std::chrono::steady_clock::now();
    Scratch w;
    KingArgs a{};
    int64_t used = 0;
    if (king_prepare(c, who, use, w, a, &used)) return 1;
    const int64_t nG = a.nG;
    a.nblocks = nG * (nG + 1) / 2;
    if (a.nblocks > KING_BLOCKS_MAX)
        return fail(c, "%s: N = %lld has more than %lld block pairs, the most one launch takes", who, (long long)c->N, (long long)KING_BLOCKS_MAX);
    a.cutoff = cutoff;
    a.cap = (unsigned long long)cap;
    KGALLOC(a.found, 1);
    KGALLOC(a.pi, (size_t)cap);
    KGALLOC(a.pj, (size_t)cap);
    KGALLOC(a.pkin, (size_t)cap);
    KGALLOC(a.pcounts, 5 * (size_t)cap);
    HIPCHK(c, hipMemsetAsync(a.found, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_king_block<EP_PAIRS>, dim3((unsigned)a.nblocks), dim3(256), 0, c->stream, a);
    KCHK(c);
    unsigned long long found = 0;
    HIPCHK(c, hipMemcpyAsync(&found, a.found, sizeof(found), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (found > 0 && found <= (unsigned long long)cap) {
        // the slots were handed out in the order the workgroups happened to ask: deliver in ascending (i, j)
        const size_t n = (size_t)found;
        std::vector<int> hi(n), hj(n), hc(5 * n);
        std::vector<double> hk(n);
        HIPCHK(c, hipMemcpyAsync(hi.data(), a.pi, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hj.data(), a.pj, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hk.data(), a.pkin, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hc.data(), a.pcounts, sizeof(int) * 5 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<size_t> ord(n);
        std::iota(ord.begin(), ord.end(), (size_t)0);
        std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return hi[x] != hi[y] ? hi[x] < hi[y] : hj[x] < hj[y]; });
        for (size_t t = 0; t < n; t++) {
            const size_t s = ord[t];
            pi[t] = hi[s];
            pj[t] = hj[s];
            kin[t] = hk[s];
            for (int q = 0; q < 5; q++) counts[5 * t + q] = hc[5 * s + q];
        }
    }
    *n_found = (int64_t)found;
    c->king_last.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->king_last.block_pairs = a.nblocks;
    c->king_last.used_markers = used;
    c->king_last.pairs = c->N * (c->N - 1) / 2;
    c->king_last.useful_macs = 5.0 * (double)used * (double)c->king_last.pairs;
    c->king_last.scratch_bytes = (double)w.bytes;
    return 0;
}

int gv_king_info(gv_ctx* c, gv_king_stats* info) {
    if (!c || !info) return 1;
    *info = c->king_last;
    return 0;
}

}  // extern "C"
