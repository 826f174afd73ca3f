// gv_dense.hip -- the dense fp64 design matrix of methylation data (type_data == "meth", data.cpp:54-57 / :107-110): marker
// statistics, data::ATx, data::Ax and their two-vector forms, and the device-side synthetic matrix.
//
// Layout: marker-major fp64 rows as the reference holds meth_data (data.cpp:245-266, meth_data[i*N + j]), the row pitch padded to
// a multiple of 64 doubles with zeros in the padding.  One layout serves both products.  Every offset is 64-bit (the reference's
// `int` products mloc * N and i * N, data.cpp:785,1022, overflow past 2^31 elements).
//
// Decomposition (closed form from N, M and the CU count, no tuning):
//   statistics / ATx : one wave per marker row, four rows per 256-thread workgroup, 16-byte non-temporal loads four deep per lane;
//                      a lane sums its pieces in ascending order, the 64 lane sums are combined by a fixed xor butterfly.
//   Ax               : a workgroup owns 512 individuals (a double2 per lane) and a segment of markers; the per-marker weights
//                      msig[i] v[i] and mave[i] are uniform across it (scalar loads).  K segments write K partial vectors that
//                      a second kernel adds in segment order -- no atomics, results are bit-reproducible run to run.
// The two-vector forms run the one-vector arithmetic per slot in the same order, so each slot is bit-identical to the
// one-vector kernel on that vector.
//
// Compact dense data (gv_upload_dosage / gv_upload_dosage_file / gv_synth_dosage): the same kind with X = scale * B, B unsigned 8- or
// 16-bit codes, marker-major, the row pitch padded to 64 codes.  Kernels of their own below (k_dosage_*): all arithmetic in code
// units -- (b - mu') per entry with mu' the mean code, the factor `scale` folded into the per-marker weight -- so that a constant
// row has q == 0 exactly whatever the scale.
//   statistics : one wave per marker row; the sum of the codes is an exact integer sum.
//   ATx        : one wave owns R consecutive rows (8 for one vector, 4 for two) and walks the individuals in steps of 1024: a lane
//                loads four 4-code pieces per row (piece k at 256 k + 4 lane, so every wave load is contiguous) and keeps its 16
//                entries of p in registers across the R rows.
//   Ax         : as the fp64 kernel with a 16-byte load per lane: 16 (u8) or 8 (u16) individuals per lane, 4096 / 2048 per workgroup.
//   assoc      : the per-marker association test (gv_assoc_*): the streaming structure of ATx with R = 4 rows per wave taken from an
//                index list, three sums per row and the regression test in the epilogue.
//
// Host side (namespace gvd, at the end): one set of launchers for the three widths.  Each takes the resident matrix as a gvd::View
// (gv_internal.h) and forks inside: bits == 0 launches the fp64 kernels, 8 / 16 go through with_codes, the one place where (bits, na)
// picks a k_dosage_* instantiation.
#include "gv_internal.h"
#include "gv_pval_dev.h"

namespace {

constexpr int WAVE = 64;
constexpr int AX_COLS = gvd::AX_COLS_F64;     // individuals per Ax workgroup: 256 lanes x one double2

__device__ inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ inline double2 ntload2(const double* p) {      // one 16-byte non-temporal load (the row is read once per pass)
    const f64x2 v = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(p));
    return make_double2(v.x, v.y);
}

__device__ inline double wave_sum(double v) {      // fixed order: the same bits on every call
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ inline double present(const uint32_t* __restrict__ mask2, int64_t n) {
    return (double)((mask2[n >> 4] >> (2 * (n & 15))) & 1u);
}

// ---- synthetic matrix: value(g, n) = c_g 2^-12 + (u0 + u1 + u2 + u3) 2^-19, with c_g an 11-bit per-marker centre and u_k the
// four 16-bit fields of a per-entry hash (an Irwin-Hall sum).  Every value is a dyadic rational of at most 20 significant bits,
// exact in fp64, so gvamp_amd/synth.py:synth_meth reproduces the matrix bit for bit.  Pad columns are written as zeros.
__global__ void k_synth_meth(double* __restrict__ A, int64_t M, int64_t S, int64_t N, int64_t pitch, uint64_t seed) {
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint64_t g = (uint64_t)(S + m);
        const uint64_t hm = splitmix64(seed ^ (g * 0xD1342543DE82EF95ull));
        const uint64_t base = splitmix64(hm + 0x632BE59BD9B4E019ull);
        const double centre = (double)(hm >> 53) * 0x1p-12;
        double* row = A + m * pitch;
        for (int64_t j = threadIdx.x; j < pitch; j += blockDim.x) {
            double v = 0.0;
            if (j < N) {
                const uint64_t r = splitmix64(base + (uint64_t)j);
                const uint64_t s = (r & 0xFFFFull) + ((r >> 16) & 0xFFFFull) + ((r >> 32) & 0xFFFFull) + (r >> 48);
                v = centre + (double)s * 0x1p-19;
            }
            row[j] = v;
        }
    }
}

// ---- compute_markers_statistics, meth branch (data.cpp:487-540): two passes over the row, as the reference does them
__global__ __launch_bounds__(256) void k_dense_stats(const double* __restrict__ A, int64_t M, int64_t N, int64_t pitch,
                                                     const uint32_t* __restrict__ mask2, double nonas, double alpha_scale,
                                                     double* __restrict__ mave, double* __restrict__ msig) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const double* row = A + m * pitch;
    double s = 0.0;
    for (int64_t j = lane; j < N; j += WAVE) s += row[j] * present(mask2, j);
    const double mu = wave_sum(s) / nonas;
    double q = 0.0;
    for (int64_t j = lane; j < N; j += WAVE) {
        const double d = (row[j] - mu) * present(mask2, j);
        q = fma(d, d, q);
    }
    q = wave_sum(q);
    if (lane == 0) {
        mave[m] = mu;
        double sg = 1.0;      // a constant column
        if (q != 0.0)
            sg = alpha_scale == 1.0 ? 1.0 / sqrt(q / (nonas - 1.0)) : 1.0 / pow(sqrt(q / (nonas - 1.0)), alpha_scale);
        msig[m] = sg;
    }
}

// ---- data::ATx, meth branch (dot_product data.cpp:783-797, ATx :814-835): out[m] = msig[m] * sum_j (x[m][j] - mave[m]) p[j]
// * scale, the difference formed inside the loop (methylation values have large means relative to their spread).  Optional
// epilogue of lmmse_mult (vamp.cpp:1112-1115): out = tau * out + gam2 * addx.
template <int NV>
__global__ __launch_bounds__(256) void k_dense_atx(const double* __restrict__ A, int64_t M, int64_t N, int64_t pitch,
                                                   const double* __restrict__ pa, const double* __restrict__ pb,
                                                   const double* __restrict__ mave, const double* __restrict__ msig,
                                                   double scale, double* __restrict__ outa, double* __restrict__ outb,
                                                   const double* __restrict__ addxa, const double* __restrict__ addxb,
                                                   double tau, double gam2) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const double* row = A + m * pitch;
    const double2* p2a = reinterpret_cast<const double2*>(pa);
    const double2* p2b = reinterpret_cast<const double2*>(pb);
    const double mu = mave[m];
    const int64_t nh = N >> 1;      // whole double2 pieces below N
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = 0.0;
    int64_t k = lane;
    for (; k + 3 * WAVE < nh; k += 4 * WAVE) {
        double2 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = ntload2(row + 2 * (k + u * WAVE));
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const double d0 = x[u].x - mu, d1 = x[u].y - mu;
            const double2 qa = p2a[k + u * WAVE];
            acc[0] = fma(d0, qa.x, acc[0]);
            acc[0] = fma(d1, qa.y, acc[0]);
            if (NV == 2) {
                const double2 qb = p2b[k + u * WAVE];
                acc[NV - 1] = fma(d0, qb.x, acc[NV - 1]);
                acc[NV - 1] = fma(d1, qb.y, acc[NV - 1]);
            }
        }
    }
    for (; k < nh; k += WAVE) {
        const double2 x = ntload2(row + 2 * k);
        const double d0 = x.x - mu, d1 = x.y - mu;
        const double2 qa = p2a[k];
        acc[0] = fma(d0, qa.x, acc[0]);
        acc[0] = fma(d1, qa.y, acc[0]);
        if (NV == 2) {
            const double2 qb = p2b[k];
            acc[NV - 1] = fma(d0, qb.x, acc[NV - 1]);
            acc[NV - 1] = fma(d1, qb.y, acc[NV - 1]);
        }
    }
    if ((N & 1) && lane == (int)(nh & (WAVE - 1))) {     // odd N: the last individual, after the lane's own pieces
        const double d = A[m * pitch + N - 1] - mu;
        acc[0] = fma(d, pa[N - 1], acc[0]);
        if (NV == 2) acc[NV - 1] = fma(d, pb[N - 1], acc[NV - 1]);
    }
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = wave_sum(acc[v]);
    if (lane == 0) {
        const double sg = msig[m];
        double r = sg * acc[0] * scale;
        outa[m] = addxa ? fma(tau, r, gam2 * addxa[m]) : r;
        if (NV == 2) {
            r = sg * acc[NV - 1] * scale;
            outb[m] = addxb ? fma(tau, r, gam2 * addxb[m]) : r;
        }
    }
}

// ---- data::Ax, meth branch (data.cpp:1013-1045), first stage: partial[seg][j] = sum over the segment's markers i of
// (x[i][j] - mave[i]) * (msig[i] v[i]), markers in ascending order.  Columns N <= j < pitch carry (0 - mave) terms that the
// reduction discards.
template <int NV>
__global__ __launch_bounds__(256) void k_dense_ax(const double* __restrict__ A, int64_t M, int64_t pitch, int64_t seg_len,
                                                  const double* __restrict__ va, const double* __restrict__ vb,
                                                  const double* __restrict__ mave, const double* __restrict__ msig,
                                                  double* __restrict__ part, int64_t part_stride, int64_t npad) {
    const int64_t col = (int64_t)blockIdx.x * AX_COLS + 2 * threadIdx.x;
    if (col >= pitch) return;
    const int64_t i0 = (int64_t)blockIdx.y * seg_len;
    const int64_t i1 = i0 + seg_len < M ? i0 + seg_len : M;
    const double* base = A + col;
    double2 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = make_double2(0.0, 0.0);
    int64_t i = i0;
    for (; i + 3 < i1; i += 4) {
        double2 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = ntload2(base + (i + u) * pitch);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const double mu = mave[i + u], sg = msig[i + u];
            const double d0 = x[u].x - mu, d1 = x[u].y - mu;
            const double wa = sg * va[i + u];
            acc[0].x = fma(d0, wa, acc[0].x);
            acc[0].y = fma(d1, wa, acc[0].y);
            if (NV == 2) {
                const double wb = sg * vb[i + u];
                acc[NV - 1].x = fma(d0, wb, acc[NV - 1].x);
                acc[NV - 1].y = fma(d1, wb, acc[NV - 1].y);
            }
        }
    }
    for (; i < i1; i++) {
        const double2 x = ntload2(base + i * pitch);
        const double mu = mave[i], sg = msig[i];
        const double d0 = x.x - mu, d1 = x.y - mu;
        const double wa = sg * va[i];
        acc[0].x = fma(d0, wa, acc[0].x);
        acc[0].y = fma(d1, wa, acc[0].y);
        if (NV == 2) {
            const double wb = sg * vb[i];
            acc[NV - 1].x = fma(d0, wb, acc[NV - 1].x);
            acc[NV - 1].y = fma(d1, wb, acc[NV - 1].y);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        *reinterpret_cast<double2*>(part + v * part_stride + (int64_t)blockIdx.y * npad + col) = acc[v];
}

// second stage: out[j] = (sum_seg partial[seg][j]) * scale in segment order for j < N, exact zeros at the pad slots j >= N.
// The phenotype mask is NOT applied: the reference's meth Ax leaves individuals with a missing phenotype unmasked.
template <int NV>
__global__ void k_dense_ax_reduce(const double* __restrict__ part, int64_t part_stride, int K, int64_t N, int64_t npad,
                                  double scale, double* __restrict__ outa, double* __restrict__ outb) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npad) return;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        double s = 0.0;
        if (j < N)
            for (int k = 0; k < K; k++) s += part[v * part_stride + (int64_t)k * npad + j];
        (v == 0 ? outa : outb)[j] = j < N ? s * scale : 0.0;
    }
}

// ================================================ compact dense data: 8- / 16-bit codes ==========================================
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Quad: four consecutive codes in one load; get(q, e) zero-extends code e (codes are unsigned: 128.. / 32768.. stay positive)
template <typename T> struct Code;
template <> struct Code<uint8_t> {
    typedef uint32_t Quad;
    static constexpr uint32_t RESERVED = 0xFFu;      // the missing entry of gv_set_dosage_missing: the all-ones code
    static __device__ inline uint32_t get(Quad q, int e) { return (q >> (8 * e)) & 0xFFu; }
    static __device__ inline uint32_t get16(const u32x4& x, int e) { return (x[e >> 2] >> (8 * (e & 3))) & 0xFFu; }
};
template <> struct Code<uint16_t> {
    typedef u32x2 Quad;
    static constexpr uint32_t RESERVED = 0xFFFFu;
    static __device__ inline uint32_t get(Quad q, int e) { return ((e < 2 ? q.x : q.y) >> (16 * (e & 1))) & 0xFFFFu; }
    static __device__ inline uint32_t get16(const u32x4& x, int e) { return (x[e >> 1] >> (16 * (e & 1))) & 0xFFFFu; }
};
template <typename T> __device__ inline typename Code<T>::Quad ntquad(const T* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const typename Code<T>::Quad*>(p));
}
// d = code - mu'; NA (gv_set_dosage_missing): the reserved code gives +0.0 instead, compared where the code is extracted.  A select,
// not a multiply: every sum below then adds an exact zero for a missing entry, and a row without one gets the bits of NA = false.
template <typename T, bool NA> __device__ inline double code_diff(uint32_t code, double mu) {
    const double d = (double)code - mu;
    if (NA) return code == Code<T>::RESERVED ? 0.0 : d;
    return d;
}

// ---- synthetic codes: genotype g in {0, 1, 2} from two allele draws at the marker's frequency (655 + h mod 32113) / 65536 -- about
// 0.01 to 0.5 -- plus an imputation-like jitter, the product of two 16-bit hash fields: code = g * 3 * 2^(bits-3) + (jitter >> (18 -
// bits)), i.e. {0, 96, 192} + [0, 63] for 8 bits and {0, 24576, 49152} + [0, 16383] for 16.  Integer arithmetic only, so
// gvamp_amd/synth.py:synth_dosage reproduces the matrix bit for bit.  Pad columns are written as zeros.
// NA (gv_synth_dosage_na): the generated code is clamped one below the reserved code, then an independent draw -- the high half of a
// second hash of the entry -- below miss_thr = miss_ppm 2^32 / 10^6 replaces it by the reserved code.
template <typename T, bool NA>
__global__ void k_synth_dosage(T* __restrict__ A, int64_t M, int64_t S, int64_t N, int64_t pitch, uint64_t seed, uint64_t miss_thr) {
    constexpr int BITS = 8 * (int)sizeof(T);
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint64_t g = (uint64_t)(S + m);
        const uint64_t hm = splitmix64(seed ^ (g * 0xD1342543DE82EF95ull));
        const uint64_t base = splitmix64(hm + 0x632BE59BD9B4E019ull);
        const uint64_t maf = 655ull + hm % 32113ull;
        T* row = A + m * pitch;
        for (int64_t j = threadIdx.x; j < pitch; j += blockDim.x) {
            uint64_t v = 0;
            if (j < N) {
                const uint64_t r = splitmix64(base + (uint64_t)j);
                const uint64_t geno = ((r & 0xFFFFull) < maf ? 1ull : 0ull) + (((r >> 16) & 0xFFFFull) < maf ? 1ull : 0ull);
                const uint64_t jit = (((r >> 32) & 0xFFFFull) * (r >> 48)) >> 16;
                v = geno * (3ull << (BITS - 3)) + (jit >> (18 - BITS));
                if (NA) {
                    if (v >= Code<T>::RESERVED) v = Code<T>::RESERVED - 1;
                    if ((splitmix64(r ^ 0x9FB21C651E98DF25ull) >> 32) < miss_thr) v = Code<T>::RESERVED;
                }
            }
            row[j] = (T)v;
        }
    }
}

// gv_synth_dosage_ld: k_synth_dosage's codes with k_synth_bed's block latent.  The markers of a block of ld_block consecutive markers
// share, per individual, one latent hash lat; an entry takes its two allele draws (the two low 16-bit fields) from lat with probability
// ld_thr / 2^32 -- decided by the high half of rs, a second hash of the entry -- and from its own hash r otherwise, and pushes them through
// the marker's own frequency: co-monotone genotypes inside a block, independent blocks.  The jitter always comes from the high half of
// r.  The code is clamped one below the reserved code; a THIRD hash below miss_thr replaces it by the reserved code, so that
// missingness is independent of the LD draw.  Integer arithmetic only (gvamp_amd/synth.py:synth_dosage_ld, bit for bit).
template <typename T>
__global__ void k_synth_dosage_ld(T* __restrict__ A, int64_t M, int64_t S, int64_t N, int64_t pitch, uint64_t seed, uint64_t miss_thr,
                                  uint64_t ld_block, uint64_t ld_thr) {
    constexpr int BITS = 8 * (int)sizeof(T);
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint64_t g = (uint64_t)(S + m);
        const uint64_t hm = splitmix64(seed ^ (g * 0xD1342543DE82EF95ull));
        const uint64_t base = splitmix64(hm + 0x632BE59BD9B4E019ull);
        const uint64_t maf = 655ull + hm % 32113ull;
        const uint64_t lbase = splitmix64(seed ^ ((g / ld_block) * 0xA24BAED4963EE407ull) ^ 0x5851F42D4C957F2Dull);
        T* row = A + m * pitch;
        for (int64_t j = threadIdx.x; j < pitch; j += blockDim.x) {
            uint64_t v = 0;
            if (j < N) {
                const uint64_t r = splitmix64(base + (uint64_t)j);
                const uint64_t rs = splitmix64(r ^ 0x9FB21C651E98DF25ull);
                const uint64_t al = (rs >> 32) < ld_thr ? splitmix64(lbase + (uint64_t)j) : r;
                const uint64_t geno = ((al & 0xFFFFull) < maf ? 1ull : 0ull) + (((al >> 16) & 0xFFFFull) < maf ? 1ull : 0ull);
                const uint64_t jit = (((r >> 32) & 0xFFFFull) * (r >> 48)) >> 16;
                v = geno * (3ull << (BITS - 3)) + (jit >> (18 - BITS));
                if (v >= Code<T>::RESERVED) v = Code<T>::RESERVED - 1;
                if ((splitmix64(rs ^ 0x2545F4914F6CDD1Dull) >> 32) < miss_thr) v = Code<T>::RESERVED;
            }
            row[j] = (T)v;
        }
    }
}

// ---- marker statistics in code units: mu' = (sum_present b) / nonas with the integer sum exact, q = sum_present (b - mu')^2 in a
// second pass; mave = scale mu', msig = 1 if q == 0 else (scale sqrt(q / (nonas - 1)))^-alpha_scale.  mu' is kept for the products.
// NA: b = 0 at the reserved code.  A second integer sum cnt = sum b na rides the butterfly of the first; mu' = (sum code b na) / cnt, 0
// when cnt == 0; q runs over the present entries; the divisor under the root stays nonas - 1, as the bed statistics divide.  cnt is
// kept in dcnt (exact in a double).  A row without the reserved code has cnt == nonas and gets the bits of NA = false.
template <typename T, bool NA>
__global__ __launch_bounds__(256) void k_dosage_stats(const T* __restrict__ A, int64_t M, int64_t N, int64_t pitch,
                                                      const uint32_t* __restrict__ mask2, double nonas, double alpha_scale,
                                                      double wscale, double* __restrict__ dmu, double* __restrict__ mave,
                                                      double* __restrict__ msig, double* __restrict__ dcnt, double* __restrict__ dq) {
    typedef typename Code<T>::Quad Quad;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const T* row = A + m * pitch;
    unsigned long long s = 0, cnt = 0;
    for (int64_t j0 = 4 * lane; j0 < N; j0 += 4 * WAVE) {      // (j0 < N <= pitch, both multiples of 4 or beyond: the piece is in the row)
        const Quad x = *reinterpret_cast<const Quad*>(row + j0);
        const uint32_t mk = mask2[j0 >> 4] >> (2 * (j0 & 15));
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (j0 + e < N) {
                const uint32_t code = Code<T>::get(x, e);
                if (NA) {
                    const uint32_t bn = code != Code<T>::RESERVED ? (mk >> (2 * e)) & 1u : 0u;
                    s += (unsigned long long)(code * bn);
                    cnt += bn;
                } else
                    s += (unsigned long long)(code * ((mk >> (2 * e)) & 1u));
            }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, WAVE);
        if (NA) cnt += __shfl_xor(cnt, off, WAVE);
    }
    const double mu = NA ? (cnt ? (double)s / (double)cnt : 0.0) : (double)s / nonas;
    double q = 0.0;
    for (int64_t j0 = 4 * lane; j0 < N; j0 += 4 * WAVE) {
        const Quad x = *reinterpret_cast<const Quad*>(row + j0);
        const uint32_t mk = mask2[j0 >> 4] >> (2 * (j0 & 15));
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (j0 + e < N) {
                const double d = code_diff<T, NA>(Code<T>::get(x, e), mu) * (double)((mk >> (2 * e)) & 1u);
                q = fma(d, d, q);
            }
    }
    q = wave_sum(q);
    if (lane == 0) {
        dmu[m] = mu;
        if (NA) dcnt[m] = (double)cnt;
        dq[m] = q;
        mave[m] = wscale * mu;
        double sg = 1.0;      // a constant column: q == 0 exactly in code units, whatever the scale
        if (q != 0.0) {
            const double sd = wscale * sqrt(q / (nonas - 1.0));
            sg = alpha_scale == 1.0 ? 1.0 / sd : 1.0 / pow(sd, alpha_scale);
        }
        msig[m] = sg;
    }
}

// ---- ATx: out[m] = (msig[m] scale_x) sum_{j<N} (b[m][j] - mu'[m]) p[j] / sqrt(N), then the lmmse_mult epilogue.  A lane's sum runs
// over its entries in ascending column step, piece and entry order whatever NV and R are, then the fixed butterfly: each slot of the
// two-vector form is bit-identical to the one-vector call.
// NA: d is +0.0 at the reserved code (code_diff), in the same place of the same order.
constexpr int ATX_STEP = 1024;      // individuals per column step of a wave: 64 lanes x 4 pieces x 4 codes
template <typename T, int NV, int R, bool NA>
__global__ __launch_bounds__(256) void k_dosage_atx(const T* __restrict__ A, int64_t M, int64_t N, int64_t pitch,
                                                    const double* __restrict__ pa, const double* __restrict__ pb,
                                                    const double* __restrict__ dmu, const double* __restrict__ msig, double wscale,
                                                    double scale, double* __restrict__ outa, double* __restrict__ outb,
                                                    const double* __restrict__ addxa, const double* __restrict__ addxb, double tau,
                                                    double gam2) {
    typedef typename Code<T>::Quad Quad;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * R;
    if (m0 >= M) return;
    const T* row[R];
    double mu[R], acc[R][NV];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t mr = m0 + r < M ? m0 + r : M - 1;      // (a row group's tail re-reads the last row; nothing is written for it)
        row[r] = A + mr * pitch + 4 * lane;
        mu[r] = dmu[mr];
#pragma unroll
        for (int v = 0; v < NV; v++) acc[r][v] = 0.0;
    }
    int64_t c0 = 0;
    for (; c0 + ATX_STEP <= N; c0 += ATX_STEP) {
        Quad x[R][4];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) x[r][k] = ntquad<T>(row[r] + c0 + 256 * k);
        double p[NV][4][4];
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double2* q = reinterpret_cast<const double2*>((v == 0 ? pa : pb) + c0 + 256 * k + 4 * lane);
                const double2 q0 = q[0], q1 = q[1];
                p[v][k][0] = q0.x; p[v][k][1] = q0.y; p[v][k][2] = q1.x; p[v][k][3] = q1.y;
            }
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const double d = code_diff<T, NA>(Code<T>::get(x[r][k], e), mu[r]);
#pragma unroll
                    for (int v = 0; v < NV; v++) acc[r][v] = fma(d, p[v][k][e], acc[r][v]);
                }
    }
    if (c0 < N) {      // the last, partial step: a piece starts below N or is skipped; j0 < N implies j0 + 3 < pitch <= npad
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t j0 = c0 + 256 * k + 4 * lane;
            if (j0 < N) {
                double p[NV][4];
#pragma unroll
                for (int v = 0; v < NV; v++)
#pragma unroll
                    for (int e = 0; e < 4; e++) p[v][e] = j0 + e < N ? (v == 0 ? pa : pb)[j0 + e] : 0.0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const Quad x = ntquad<T>(row[r] + c0 + 256 * k);
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (j0 + e < N) {
                            const double d = code_diff<T, NA>(Code<T>::get(x, e), mu[r]);
#pragma unroll
                            for (int v = 0; v < NV; v++) acc[r][v] = fma(d, p[v][e], acc[r][v]);
                        }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int v = 0; v < NV; v++) acc[r][v] = wave_sum(acc[r][v]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t m = m0 + r;
            if (m < M) {
                const double w = msig[m] * wscale;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const double res = w * acc[r][v] * scale;
                    const double* addx = v == 0 ? addxa : addxb;
                    (v == 0 ? outa : outb)[m] = addx ? fma(tau, res, gam2 * addx[m]) : res;
                }
            }
        }
    }
}

// ---- association test (gv_assoc_*; data::pvals_calc / pvals_calc_LOCO restated for codes with b == 1).  First the residual:
// p = y - z1 (+ add) at the individuals with a phenotype, 0 at NA and pad slots whatever the caller left in y, and the block partials
// {sum p, sum p^2} (K = 2) that gvk::finalize adds up in its fixed order.  The grid depends on npad alone.
__global__ __launch_bounds__(256) void k_assoc_prep(const double* __restrict__ y, const double* __restrict__ z1,
                                                    const double* __restrict__ add, const uint32_t* __restrict__ mask2, int64_t npad,
                                                    double* __restrict__ p, double* __restrict__ partial) {
    __shared__ double sh[2][4];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < npad; j += (int64_t)gridDim.x * 256) {
        double v = 0.0;
        if ((mask2[j >> 4] >> (2 * (j & 15))) & 1u) {
            v = y[j] - z1[j];
            if (add) v += add[j];
        }
        p[j] = v;
        s1 += v;
        s2 = fma(v, v, s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & (WAVE - 1)) == 0) { sh[0][threadIdx.x >> 6] = s1; sh[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}

// The marker pass: one wave owns R rows of the index list `rows` (NULL: the identity) and walks the individuals as k_dosage_atx does.
// Per row three sums with d = code - mu' formed per entry: sum d p, sum d na, sum (d na) d, each over the lane's entries in ascending
// column step, piece and entry order, then the fixed butterfly -- a row's bits depend neither on R nor on the group or the list it
// arrives in.  (d na) is a select: d * 1 and d * 0 of a finite d, without the multiply.  Lane 0 runs the test (gvp::dosage_stats).
// NA: d is +0.0 at the reserved code, and two more sums per row, sum b p and sum b p^2 of the masked residual, stand where the
// pass's totals sp, sp2 stand otherwise; the sample size is the count the statistics left in dcnt.  A row whose count is nonas misses
// nobody with a phenotype: its sums ARE sp and sp2, which it takes -- the bits of NA = false.
template <typename T, int R, bool NA>
__global__ __launch_bounds__(256) void k_dosage_assoc(const T* __restrict__ A, int64_t N, int64_t pitch, const int64_t* __restrict__ rows,
                                                      int64_t nrows, const double* __restrict__ p, const uint32_t* __restrict__ mask2,
                                                      const double* __restrict__ dmu, const double* __restrict__ msig, double wscale,
                                                      const double* __restrict__ psums, double nonas, const double* __restrict__ dcnt,
                                                      const double* __restrict__ xself, double self_scale, double* __restrict__ beta,
                                                      double* __restrict__ se, double* __restrict__ tstat, double* __restrict__ pval) {
    typedef typename Code<T>::Quad Quad;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * R;
    if (i0 >= nrows) return;
    const T* row[R];
    constexpr int NS = NA ? 5 : 3;
    double mu[R], acc[R][NS];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t ir = i0 + r < nrows ? i0 + r : nrows - 1;      // (a group's tail re-reads the last row; nothing is written for it)
        const int64_t mr = rows ? rows[ir] : ir;
        row[r] = A + mr * pitch + 4 * lane;
        mu[r] = dmu[mr];
#pragma unroll
        for (int v = 0; v < NS; v++) acc[r][v] = 0.0;
    }
    int64_t c0 = 0;
    for (; c0 + ATX_STEP <= N; c0 += ATX_STEP) {
        Quad x[R][4];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) x[r][k] = ntquad<T>(row[r] + c0 + 256 * k);
        double q[4][4];
        uint32_t mk[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t j0 = c0 + 256 * k + 4 * lane;
            const double2* q2 = reinterpret_cast<const double2*>(p + j0);
            const double2 q0 = q2[0], q1 = q2[1];
            q[k][0] = q0.x; q[k][1] = q0.y; q[k][2] = q1.x; q[k][3] = q1.y;
            mk[k] = mask2[j0 >> 4] >> (2 * (j0 & 15));
        }
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t code = Code<T>::get(x[r][k], e);
                    const double d = code_diff<T, NA>(code, mu[r]);
                    const double dn = (mk[k] >> (2 * e)) & 1u ? d : 0.0;
                    acc[r][0] = fma(d, q[k][e], acc[r][0]);
                    acc[r][1] += dn;
                    acc[r][2] = fma(dn, d, acc[r][2]);
                    if (NA) {
                        const double pb = code == Code<T>::RESERVED ? 0.0 : q[k][e];
                        acc[r][NS - 2] += pb;
                        acc[r][NS - 1] = fma(pb, pb, acc[r][NS - 1]);
                    }
                }
    }
    if (c0 < N) {      // the last, partial step: a piece starts below N or is skipped; j0 < N implies j0 + 3 < pitch <= npad
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t j0 = c0 + 256 * k + 4 * lane;
            if (j0 < N) {
                double q[4];
#pragma unroll
                for (int e = 0; e < 4; e++) q[e] = j0 + e < N ? p[j0 + e] : 0.0;
                const uint32_t mk = mask2[j0 >> 4] >> (2 * (j0 & 15));
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const Quad x = ntquad<T>(row[r] + c0 + 256 * k);
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (j0 + e < N) {
                            const uint32_t code = Code<T>::get(x, e);
                            const double d = code_diff<T, NA>(code, mu[r]);
                            const double dn = (mk >> (2 * e)) & 1u ? d : 0.0;
                            acc[r][0] = fma(d, q[e], acc[r][0]);
                            acc[r][1] += dn;
                            acc[r][2] = fma(dn, d, acc[r][2]);
                            if (NA) {
                                const double pb = code == Code<T>::RESERVED ? 0.0 : q[e];
                                acc[r][NS - 2] += pb;
                                acc[r][NS - 1] = fma(pb, pb, acc[r][NS - 1]);
                            }
                        }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int v = 0; v < NS; v++) acc[r][v] = wave_sum(acc[r][v]);
    if (lane == 0) {
        const double sp = psums[0], sp2 = psums[1];
#pragma unroll
        for (int r = 0; r < R; r++)
            if (i0 + r < nrows) {
                const int64_t m = rows ? rows[i0 + r] : i0 + r;
                const double cself = xself ? xself[m] * self_scale : 0.0;
                gvp::Reg1d res;
                if (NA) {      // sample size cnt_k; fewer than three present individuals leave no test
                    const double n = dcnt[m];
                    const bool whole = n == nonas;
                    res = gvp::dosage_stats(acc[r][0], acc[r][1], acc[r][2], msig[m] * wscale, whole ? sp : acc[r][NS - 2],
                                            whole ? sp2 : acc[r][NS - 1], n, cself);
                    if (n < 3.0) res.beta = res.se = res.t = res.p = __builtin_nan("");
                } else
                    res = gvp::dosage_stats(acc[r][0], acc[r][1], acc[r][2], msig[m] * wscale, sp, sp2, nonas, cself);
                beta[m] = res.beta; se[m] = res.se; tstat[m] = res.t; pval[m] = res.p;
            }
    }
}

// ---- Ax, first stage: partial[seg][j] = sum over the segment's markers i of (b[i][j] - mu'[i]) * (msig[i] scale_x v[i]), markers in
// ascending order; a lane owns the 16 / sizeof(T) individuals of one 16-byte load.  Second stage: k_dense_ax_reduce.
// NA: (b - mu') is +0.0 at the reserved code (code_diff): the entry adds an exact zero.
template <typename T, int NV, bool NA>
__global__ __launch_bounds__(256) void k_dosage_ax(const T* __restrict__ A, int64_t M, int64_t pitch, int64_t seg_len,
                                                   const double* __restrict__ va, const double* __restrict__ vb,
                                                   const double* __restrict__ dmu, const double* __restrict__ msig, double wscale,
                                                   double* __restrict__ part, int64_t part_stride, int64_t npad) {
    constexpr int EPL = 16 / (int)sizeof(T);
    const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) * EPL;
    if (col >= pitch) return;      // (pitch is a multiple of 64: col < pitch implies col + EPL <= pitch <= npad)
    const int64_t i0 = (int64_t)blockIdx.y * seg_len;
    const int64_t i1 = i0 + seg_len < M ? i0 + seg_len : M;
    const T* base = A + col;
    double acc[NV][EPL];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[v][e] = 0.0;
    int64_t i = i0;
    for (; i + 3 < i1; i += 4) {
        u32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base + (i + u) * pitch));
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const double mu = dmu[i + u], sw = msig[i + u] * wscale;
            const double wa = sw * va[i + u], wb = sw * vb[i + u];
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double d = code_diff<T, NA>(Code<T>::get16(x[u], e), mu);
                acc[0][e] = fma(d, wa, acc[0][e]);
                if (NV == 2) acc[NV - 1][e] = fma(d, wb, acc[NV - 1][e]);
            }
        }
    }
    for (; i < i1; i++) {
        const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base + i * pitch));
        const double mu = dmu[i], sw = msig[i] * wscale;
        const double wa = sw * va[i], wb = sw * vb[i];
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            const double d = code_diff<T, NA>(Code<T>::get16(x, e), mu);
            acc[0][e] = fma(d, wa, acc[0][e]);
            if (NV == 2) acc[NV - 1][e] = fma(d, wb, acc[NV - 1][e]);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
        double2* dst = reinterpret_cast<double2*>(part + v * part_stride + (int64_t)blockIdx.y * npad + col);
#pragma unroll
        for (int e = 0; e < EPL; e += 2) dst[e >> 1] = make_double2(acc[v][e], acc[v][e + 1]);
    }
}

inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// the fp64 launches of gvd::atx / gvd::ax_partial (M > 0)
void atx_f64(hipStream_t s, int nv, const gvd::View& v, const double* pa, const double* pb, double scale, double* outa, double* outb,
             const double* addxa, const double* addxb, double tau, double gam2) {
    const double* A = (const double*)v.rows;
    if (nv == 2)
        hipLaunchKernelGGL(k_dense_atx<2>, dim3(nblk(v.M, 4)), dim3(256), 0, s, A, v.M, v.N, v.pitch, pa, pb, v.centre, v.msig, scale, outa,
                           outb, addxa, addxb, tau, gam2);
    else
        hipLaunchKernelGGL(k_dense_atx<1>, dim3(nblk(v.M, 4)), dim3(256), 0, s, A, v.M, v.N, v.pitch, pa, pa, v.centre, v.msig, scale, outa,
                           outa, addxa, addxa, tau, gam2);
}
void ax_partial_f64(hipStream_t s, int nv, const gvd::AxShape& sh, const gvd::View& v, const double* va, const double* vb, double* part,
                    int64_t stride, int64_t npad) {
    const double* A = (const double*)v.rows;
    const dim3 grid((unsigned)sh.col_tiles, (unsigned)sh.segs);
    if (nv == 2)
        hipLaunchKernelGGL(k_dense_ax<2>, grid, dim3(256), 0, s, A, v.M, v.pitch, sh.seg_len, va, vb, v.centre, v.msig, part, stride, npad);
    else
        hipLaunchKernelGGL(k_dense_ax<1>, grid, dim3(256), 0, s, A, v.M, v.pitch, sh.seg_len, va, va, v.centre, v.msig, part, stride, npad);
}

// The one place where (bits, na) picks the instantiation of a k_dosage_* kernel: f is called with a CodeKind carrying the code type
// and whether the all-ones code is a missing entry.
template <typename T, bool NA> struct CodeKind { typedef T type; static constexpr bool na = NA; };
template <typename F> void with_codes(int bits, bool na, F&& f) {
    if (bits == 8) {
        if (na) f(CodeKind<uint8_t, true>()); else f(CodeKind<uint8_t, false>());
    } else {
        if (na) f(CodeKind<uint16_t, true>()); else f(CodeKind<uint16_t, false>());
    }
}

}  // namespace

namespace gvd {

int64_t row_pitch(int64_t N) { return (N + 63) / 64 * 64; }

int ax_cols(int bits) { return bits == 8 ? 4096 : (bits == 16 ? 2048 : AX_COLS); }

AxShape ax_shape(int64_t N, int64_t M, int cus, int cols) {
    AxShape sh;
    const int64_t pitch = row_pitch(N);
    sh.col_tiles = (pitch + cols - 1) / cols;
    // about eight workgroups per CU in all, every segment at least 16 markers long
    int64_t k = ((int64_t)8 * (cus > 0 ? cus : 256) + sh.col_tiles - 1) / sh.col_tiles;
    const int64_t kmax = (M + 15) / 16;
    if (k > kmax) k = kmax;
    if (k < 1) k = 1;
    sh.seg_len = M > 0 ? (M + k - 1) / k : 1;
    sh.segs = M > 0 ? (int)((M + sh.seg_len - 1) / sh.seg_len) : 1;
    return sh;
}

// (the fp64 launches stand ahead of the first code dispatch: kernels are emitted in the order of their first use)
void ax_reduce(hipStream_t s, int nv, const AxShape& sh, const double* part, int64_t N, int64_t npad, double scale, double* outa,
               double* outb) {
    const int64_t stride = (int64_t)sh.segs * npad;
    if (nv == 2)
        hipLaunchKernelGGL(k_dense_ax_reduce<2>, dim3(nblk(npad, 256)), dim3(256), 0, s, part, stride, sh.segs, N, npad, scale,
                           outa, outb);
    else
        hipLaunchKernelGGL(k_dense_ax_reduce<1>, dim3(nblk(npad, 256)), dim3(256), 0, s, part, stride, sh.segs, N, npad, scale,
                           outa, outa);
}

void synth(hipStream_t s, const View& v, int64_t S, uint64_t seed, uint64_t miss_thr) {
    const int64_t M = v.M, N = v.N, pitch = v.pitch;
    if (M <= 0) return;
    const dim3 g((unsigned)(M < 16384 ? M : 16384));
    if (!v.bits) {
        hipLaunchKernelGGL(k_synth_meth, g, dim3(256), 0, s, (double*)v.rows, M, S, N, pitch, seed);
        return;
    }
    with_codes(v.bits, v.na, [&](auto kind) {
        typedef typename decltype(kind)::type T;
        hipLaunchKernelGGL((k_synth_dosage<T, decltype(kind)::na>), g, dim3(256), 0, s, (T*)v.rows, M, S, N, pitch, seed, miss_thr);
    });
}

void synth_ld(hipStream_t s, const View& v, int64_t S, uint64_t seed, uint64_t miss_thr, uint64_t ld_block, uint64_t ld_thr) {
    if (v.M <= 0) return;
    const dim3 g((unsigned)(v.M < 16384 ? v.M : 16384));
    if (v.bits == 8)
        hipLaunchKernelGGL(k_synth_dosage_ld<uint8_t>, g, dim3(256), 0, s, (uint8_t*)v.rows, v.M, S, v.N, v.pitch, seed, miss_thr, ld_block, ld_thr);
    else
        hipLaunchKernelGGL(k_synth_dosage_ld<uint16_t>, g, dim3(256), 0, s, (uint16_t*)v.rows, v.M, S, v.N, v.pitch, seed, miss_thr, ld_block, ld_thr);
}

void stats(hipStream_t s, const View& v, const uint32_t* mask2, double nonas, double alpha_scale, double* mave) {
    const int64_t M = v.M, N = v.N, pitch = v.pitch;
    if (M <= 0) return;
    if (!v.bits) {
        hipLaunchKernelGGL(k_dense_stats, dim3(nblk(M, 4)), dim3(256), 0, s, (const double*)v.rows, M, N, pitch, mask2, nonas, alpha_scale,
                           mave, v.msig);
        return;
    }
    with_codes(v.bits, v.na, [&](auto kind) {
        typedef typename decltype(kind)::type T;
        hipLaunchKernelGGL((k_dosage_stats<T, decltype(kind)::na>), dim3(nblk(M, 4)), dim3(256), 0, s, (const T*)v.rows, M, N, pitch, mask2,
                           nonas, alpha_scale, v.wscale, v.centre, mave, v.msig, v.cnt, v.qss);
    });
}

void atx(hipStream_t s, int nv, const View& v, const double* pa, const double* pb, double scale, double* outa, double* outb,
         const double* addxa, const double* addxb, double tau, double gam2) {
    const int64_t M = v.M, N = v.N, pitch = v.pitch;
    if (M <= 0) return;
    if (!v.bits) return atx_f64(s, nv, v, pa, pb, scale, outa, outb, addxa, addxb, tau, gam2);
    with_codes(v.bits, v.na, [&](auto kind) {
        typedef typename decltype(kind)::type T;
        constexpr bool NA = decltype(kind)::na;
        const T* A = (const T*)v.rows;
        if (nv == 2)
            hipLaunchKernelGGL((k_dosage_atx<T, 2, 4, NA>), dim3(nblk(M, 16)), dim3(256), 0, s, A, M, N, pitch, pa, pb, v.centre, v.msig,
                               v.wscale, scale, outa, outb, addxa, addxb, tau, gam2);
        else {
            // (NA on 16-bit codes: R = 8 costs 151 VGPRs and 30 spilled SGPRs, so four rows per wave there; a row's bits do not depend on R)
            constexpr int R1 = NA && sizeof(T) == 2 ? 4 : 8;
            hipLaunchKernelGGL((k_dosage_atx<T, 1, R1, NA>), dim3(nblk(M, 4 * R1)), dim3(256), 0, s, A, M, N, pitch, pa, pa, v.centre, v.msig,
                               v.wscale, scale, outa, outa, addxa, addxa, tau, gam2);
        }
    });
}

void ax_partial(hipStream_t s, int nv, const AxShape& sh, const View& v, const double* va, const double* vb, double* part, int64_t npad) {
    const int64_t M = v.M, pitch = v.pitch;
    if (M <= 0) return;
    const int64_t stride = (int64_t)sh.segs * npad;
    const dim3 grid((unsigned)sh.col_tiles, (unsigned)sh.segs);
    if (!v.bits) return ax_partial_f64(s, nv, sh, v, va, vb, part, stride, npad);
    with_codes(v.bits, v.na, [&](auto kind) {
        typedef typename decltype(kind)::type T;
        constexpr bool NA = decltype(kind)::na;
        const T* A = (const T*)v.rows;
        if (nv == 2)
            hipLaunchKernelGGL((k_dosage_ax<T, 2, NA>), grid, dim3(256), 0, s, A, M, pitch, sh.seg_len, va, vb, v.centre, v.msig, v.wscale,
                               part, stride, npad);
        else
            hipLaunchKernelGGL((k_dosage_ax<T, 1, NA>), grid, dim3(256), 0, s, A, M, pitch, sh.seg_len, va, va, v.centre, v.msig, v.wscale,
                               part, stride, npad);
    });
}

constexpr int ASSOC_R = 4;
void assoc_prep(hipStream_t s, const double* y, const double* z1, const double* add, const uint32_t* mask2, int64_t npad, double* p,
                double* partial, double* sums) {
    const int64_t b = (npad + 255) / 256;
    const int nb = (int)(b < 1 ? 1 : (b > RED_BLOCKS ? RED_BLOCKS : b));
    hipLaunchKernelGGL(k_assoc_prep, dim3(nb), dim3(256), 0, s, y, z1, add, mask2, npad, p, partial);
    gvk::finalize(s, partial, nb, 2, sums);
}

void assoc(hipStream_t s, const View& v, const int64_t* rows, int64_t nrows, const double* p, const uint32_t* mask2, const double* psums,
           double nonas, const double* xself, double self_scale, double* beta, double* se, double* tstat, double* pval) {
    if (nrows <= 0) return;
    with_codes(v.bits, v.na, [&](auto kind) {
        typedef typename decltype(kind)::type T;
        hipLaunchKernelGGL((k_dosage_assoc<T, ASSOC_R, decltype(kind)::na>), dim3(nblk(nrows, 4 * ASSOC_R)), dim3(256), 0, s,
                           (const T*)v.rows, v.N, v.pitch, rows, nrows, p, mask2, v.centre, v.msig, v.wscale, psums, nonas, v.cnt, xself,
                           self_scale, beta, se, tstat, pval);
    });
}

// The reserved codes of n consecutive codes (whole pitched rows of an upload: the zero padding is not the reserved code): a count per
// lane, the fixed butterfly, the four wave counts of a block in order, then one block adds the block partials strided and by a fixed
// tree and adds the result to *total -- in stream order after the copy it counts, exact integers, no atomics.
template <typename T>
__global__ __launch_bounds__(256) void k_count_reserved(const T* __restrict__ A, int64_t n, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long sh[4];
    unsigned long long cnt = 0;
    constexpr int EPL = 16 / (int)sizeof(T);      // (n is a multiple of the row pitch, 64 codes: whole 16-byte pieces)
    const u32x4* A4 = reinterpret_cast<const u32x4*>(A);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n / EPL; j += (int64_t)gridDim.x * 256) {
        const u32x4 x = A4[j];
#pragma unroll
        for (int e = 0; e < EPL; e++) cnt += Code<T>::get16(x, e) == Code<T>::RESERVED ? 1u : 0u;
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void k_count_finish(const unsigned long long* __restrict__ partial, int nb,
                                                      unsigned long long* __restrict__ total) {
    __shared__ unsigned long long sh[256];
    unsigned long long cnt = 0;
    for (int b = threadIdx.x; b < nb; b += 256) cnt += partial[b];
    sh[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total += sh[0];
}
void count_reserved(hipStream_t s, const View& v, int64_t m0, int64_t mc, unsigned long long* partial, unsigned long long* total) {
    const int64_t n = mc * v.pitch;
    if (n <= 0) return;
    const int64_t b = (n / 8 + 255) / 256;
    const int nb = (int)(b > COUNT_BLOCKS ? COUNT_BLOCKS : b);
    with_codes(v.bits, false, [&](auto kind) {      // (the count does not depend on na)
        typedef typename decltype(kind)::type T;
        hipLaunchKernelGGL(k_count_reserved<T>, dim3(nb), dim3(256), 0, s, (const T*)v.rows + m0 * v.pitch, n, partial);
    });
    hipLaunchKernelGGL(k_count_finish, dim3(1), dim3(256), 0, s, partial, nb, total);
}

}  // namespace gvd
