// gv_pca.hip -- principal components of the resident genotypes by block subspace iteration: gv_pca_dev,
// gv_pca_loadings_dev, gv_pca_info.
//
// The two batch products (gv_atxm.hip, gv_score.hip) are called as they are; this file is everything between two products.  A panel
// is L <= 32 separate fp64 columns of npad doubles, handed to the kernels as an array of column pointers (struct Panel, by value).
//
//   k_pca_gram<T>      XtY (or XtX) of two panels into per-block L x L partial sums.  A block owns a fixed run of 64-row chunks, stages
//                      a chunk of both panels in LDS (read once, coalesced along n) and every thread holds a T x T register tile of
//                      the output.  The grid is gram_blocks(npad): the summation order of an entry is a function of (npad, L) alone.
//   k_pca_gram_fin     the block partials added in a fixed order, 32 threads per entry.  No atomics anywhere in this file.
//   k_pca_small        one workgroup, the L x L matrix in LDS, fp64: symmetrise, then either Cholesky (failure flag) and the inverse of
//                      the triangular factor, or cyclic Jacobi in a fixed round-robin order and the eigenvalues sorted descending.
//   k_pca_apply<LM>    Out = X W for an L x L' matrix W held in LDS, one thread per row; the row of X is in registers before the first
//                      store, so Out may be X.  For the residual panel the - U diag(theta) term is fused.
//   k_pca_decide       theta[0..k), r[0..k) (the square roots of the residual panel's Gram diagonal) and the Cholesky flag into the
//                      context's reduction scalars: the one read-back of an iteration.
//   k_pca_scale, k_pca_amax, k_pca_emit   column scaling; the sign rule (largest magnitude positive, lowest index on ties).
#include <chrono>
#include <cmath>
#include <cstring>

#include "gv_internal.h"

using namespace gvi;

namespace {

constexpr int LMAX = GV_PCA_MAX_BLOCK;
constexpr int GRAM_ROWS = 64;          // rows of a chunk staged in LDS
constexpr int GRAM_BLOCKS = 1024;      // most blocks of a Gram launch
constexpr int AMAX_BLOCKS = 256;       // most blocks per column of the sign rule's search (= the threads that reduce them)
constexpr int SMALL_LD = LMAX + 1;     // leading dimension of the LDS matrices of k_pca_small
constexpr int JACOBI_SWEEPS = 30;
// a Cholesky pivot at the rounding level of its own diagonal entry counts as not positive: d <= PIVOT_EPS * s_jj
constexpr double PIVOT_EPS = 32.0 * 2.220446049250313e-16;

struct Panel { double* p[LMAX]; };
struct Factors { double v[LMAX]; };

inline int nblk(int64_t n, int per) { return (int)((n + per - 1) / per); }
inline int gram_blocks(int64_t npad) {
    const int64_t chunks = (npad + GRAM_ROWS - 1) / GRAM_ROWS;
    return (int)(chunks < GRAM_BLOCKS ? chunks : GRAM_BLOCKS);
}

template <int T>
__global__ __launch_bounds__(256) void k_pca_gram(Panel X, Panel Y, int L, int64_t npad, int64_t chunks, int64_t per_block,
                                                   double* __restrict__ part) {
    constexpr int LM = 16 * T, LD = LM + 1;
    __shared__ double xs[GRAM_ROWS * LD];
    __shared__ double ys[GRAM_ROWS * LD];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15, r = t & 63;
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; a++)
#pragma unroll
        for (int b = 0; b < T; b++) acc[a][b] = 0.0;
    const int64_t c0 = (int64_t)blockIdx.x * per_block;
    const int64_t c1 = c0 + per_block < chunks ? c0 + per_block : chunks;
    // this thread's share of a chunk: row r, columns (t >> 6) + 4 q.  The next chunk is loaded into registers while this one is summed
    constexpr int NQ = LM / 4;
    double xr[NQ], yr[NQ];
    auto fetch = [&](int64_t ch) {
        const int64_t n = ch * GRAM_ROWS + r;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int col = (t >> 6) + 4 * q;
            const bool in = col < L && n < npad;
            xr[q] = in ? X.p[col][n] : 0.0;
            yr[q] = in ? Y.p[col][n] : 0.0;
        }
    };
    if (c0 < c1) fetch(c0);
    for (int64_t ch = c0; ch < c1; ch++) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            xs[r * LD + (t >> 6) + 4 * q] = xr[q];
            ys[r * LD + (t >> 6) + 4 * q] = yr[q];
        }
        __syncthreads();
        if (ch + 1 < c1) fetch(ch + 1);
#pragma unroll 4
        for (int q = 0; q < GRAM_ROWS; q++) {
            double xv[T], yv[T];
#pragma unroll
            for (int a = 0; a < T; a++) {
                xv[a] = xs[q * LD + ti + 16 * a];
                yv[a] = ys[q * LD + tj + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < T; a++)
#pragma unroll
                for (int b = 0; b < T; b++) acc[a][b] = fma(xv[a], yv[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < T; a++)
#pragma unroll
        for (int b = 0; b < T; b++) part[(int64_t)blockIdx.x * LM * LM + (ti + 16 * a) * LM + tj + 16 * b] = acc[a][b];
}

// The block partials of an entry added in a fixed order: 32 threads an entry, thread g of them adds the partials [g per, (g + 1) per) in
// block order, per = ceil(nb / 32), then the 32 sums meet in a fixed tree.  A block is 32 entries x 32 such threads, consecutive lanes on
// consecutive entries, so that a wave's load is one run of 32 doubles.
__global__ __launch_bounds__(1024) void k_pca_gram_fin(const double* __restrict__ part, int nb, int entries, double* __restrict__ S) {
    __shared__ double sm[1024];
    const int t = threadIdx.x, g = t >> 5;
    const int e = blockIdx.x * 32 + (t & 31);
    const int per = (nb + 31) / 32;
    const int b1 = (g + 1) * per < nb ? (g + 1) * per : nb;
    double s = 0.0;
    if (e < entries)
        for (int b = g * per; b < b1; b++) s += part[(int64_t)b * entries + e];
    sm[t] = s;
    __syncthreads();
    for (int w = 16; w > 0; w >>= 1) {
        if (g < w) sm[t] += sm[t + 32 * w];
        __syncthreads();
    }
    if (g == 0 && e < entries) S[e] = sm[t];
}

// mode 0: S = R^T R, W = R^-1 (upper triangular), *flag = 1 when a pivot is not positive (W = 0 then).
// mode 1: S = V Theta V^T, W = V with the columns in descending order of theta.
// S and W are LM x LM row-major; W and theta are zero beyond L.
__global__ __launch_bounds__(64) void k_pca_small(int mode, const double* __restrict__ S, int L, int LM, double* __restrict__ W,
                                                   double* __restrict__ theta, int* __restrict__ flag) {
    __shared__ double A[LMAX * SMALL_LD];
    __shared__ double V[LMAX * SMALL_LD];
    __shared__ double d0[LMAX], cs[LMAX / 2], sn[LMAX / 2];
    __shared__ int pp[LMAX / 2], qq[LMAX / 2], perm[LMAX];
    __shared__ double piv;
    __shared__ int bad, rotated;
    const int t = threadIdx.x;
    for (int e = t; e < LMAX * SMALL_LD; e += 64) { A[e] = 0.0; V[e] = 0.0; }
    if (t < LMAX) perm[t] = t < L ? t : 0;
    if (t == 0) { bad = 0; rotated = 0; }
    __syncthreads();
    for (int e = t; e < L * L; e += 64) {
        const int i = e / L, j = e % L;
        A[i * SMALL_LD + j] = 0.5 * (S[i * LM + j] + S[j * LM + i]);
    }
    __syncthreads();
    if (mode == 0) {
        if (t < L) d0[t] = A[t * SMALL_LD + t];
        __syncthreads();
        for (int j = 0; j < L; j++) {
            if (t == 0) {
                const double d = A[j * SMALL_LD + j];
                const bool ok = d > PIVOT_EPS * d0[j] && d > 0.0 && d < INFINITY;
                if (!ok) bad = 1;
                piv = ok ? sqrt(d) : 1.0;
                A[j * SMALL_LD + j] = piv;
            }
            __syncthreads();
            if (bad) break;
            const double rj = piv;
            for (int i = j + 1 + t; i < L; i += 64) A[j * SMALL_LD + i] /= rj;
            __syncthreads();
            const int m = L - j - 1;
            for (int e = t; e < m * m; e += 64) {
                const int a = j + 1 + e / m, b = j + 1 + e % m;
                if (b >= a) A[a * SMALL_LD + b] = fma(-A[j * SMALL_LD + a], A[j * SMALL_LD + b], A[a * SMALL_LD + b]);
            }
            __syncthreads();
        }
        __syncthreads();
        if (!bad && t < L) {               // column t of R^-1 by back substitution
            V[t * SMALL_LD + t] = 1.0 / A[t * SMALL_LD + t];
            for (int i = t - 1; i >= 0; i--) {
                double s = 0.0;
                for (int m = i + 1; m <= t; m++) s = fma(A[i * SMALL_LD + m], V[m * SMALL_LD + t], s);
                V[i * SMALL_LD + t] = -s / A[i * SMALL_LD + i];
            }
        }
        __syncthreads();
        const bool failed = bad != 0;
        for (int e = t; e < LM * LM; e += 64) {
            const int i = e / LM, j = e % LM;
            W[e] = (!failed && i < L && j < L && i <= j) ? V[i * SMALL_LD + j] : 0.0;
        }
        if (failed && t == 0) *flag = 1;
        return;
    }
    // cyclic Jacobi, round-robin order: step s of a sweep rotates the n2 / 2 disjoint pairs of the circle method
    for (int i = t; i < L; i += 64) V[i * SMALL_LD + i] = 1.0;
    __syncthreads();
    const int n2 = (L + 1) / 2 * 2, np = n2 / 2;
    for (int sweep = 0; sweep < JACOBI_SWEEPS && L > 1; sweep++) {
        for (int step = 0; step < n2 - 1; step++) {
            if (t < np) {
                int a, b;
                if (t == 0) { a = n2 - 1; b = step; }
                else { a = (step + t) % (n2 - 1); b = (step - t + (n2 - 1)) % (n2 - 1); }
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0;
                int act = 0;
                if (q < L) {
                    const double app = A[p * SMALL_LD + p], aqq = A[q * SMALL_LD + q], apq = A[p * SMALL_LD + q];
                    if (fabs(apq) > 2.220446049250313e-16 * sqrt(fabs(app) * fabs(aqq)) && apq != 0.0) {
                        const double th = (aqq - app) / (2.0 * apq);
                        const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(fma(th, th, 1.0)));
                        c = 1.0 / sqrt(fma(tt, tt, 1.0));
                        s = tt * c;
                        act = 1;
                        rotated = 1;
                    }
                }
                pp[t] = act ? p : -1;
                qq[t] = q;
                cs[t] = c;
                sn[t] = s;
            }
            __syncthreads();
            for (int e = t; e < np * L; e += 64) {          // A <- A J, V <- V J
                const int m = e / L, i = e % L, p = pp[m], q = qq[m];
                if (p < 0) continue;
                const double c = cs[m], s = sn[m];
                const double aip = A[i * SMALL_LD + p], aiq = A[i * SMALL_LD + q];
                A[i * SMALL_LD + p] = c * aip - s * aiq;
                A[i * SMALL_LD + q] = s * aip + c * aiq;
                const double vip = V[i * SMALL_LD + p], viq = V[i * SMALL_LD + q];
                V[i * SMALL_LD + p] = c * vip - s * viq;
                V[i * SMALL_LD + q] = s * vip + c * viq;
            }
            __syncthreads();
            for (int e = t; e < np * L; e += 64) {          // A <- J^T A
                const int m = e / L, j = e % L, p = pp[m], q = qq[m];
                if (p < 0) continue;
                const double c = cs[m], s = sn[m];
                const double apj = A[p * SMALL_LD + j], aqj = A[q * SMALL_LD + j];
                A[p * SMALL_LD + j] = c * apj - s * aqj;
                A[q * SMALL_LD + j] = s * apj + c * aqj;
            }
            __syncthreads();
        }
        const int any = rotated;
        __syncthreads();
        if (t == 0) rotated = 0;
        __syncthreads();
        if (!any) break;
    }
    if (t < L) {                            // descending order, ties by index
        const double mine = A[t * SMALL_LD + t];
        int rank = 0;
        for (int j = 0; j < L; j++) {
            const double o = A[j * SMALL_LD + j];
            rank += (o > mine || (o == mine && j < t)) ? 1 : 0;
        }
        if (rank < L) perm[rank] = t;
    }
    __syncthreads();
    for (int e = t; e < LM * LM; e += 64) {
        const int i = e / LM, j = e % LM;
        W[e] = (i < L && j < L) ? V[i * SMALL_LD + perm[j]] : 0.0;
    }
    if (t < LM) theta[t] = t < L ? A[perm[t] * SMALL_LD + perm[t]] : 0.0;
}

template <int LM>
__global__ __launch_bounds__(256) void k_pca_apply(Panel X, const double* __restrict__ W, int L, int Lout, Panel Sub,
                                                    const double* __restrict__ theta, int has_sub, Panel Out, int64_t npad) {
    __shared__ double ws[LM * LM];
    __shared__ double th[LM];
    for (int e = threadIdx.x; e < LM * LM; e += 256) ws[e] = W[e];
    if (threadIdx.x < LM) th[threadIdx.x] = has_sub ? theta[threadIdx.x] : 0.0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    double x[LM];
#pragma unroll
    for (int i = 0; i < LM; i++) x[i] = i < L ? X.p[i][n] : 0.0;
    for (int j = 0; j < Lout; j++) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < LM; i++) acc = fma(x[i], ws[i * LM + j], acc);
        if (has_sub) acc = fma(-Sub.p[j][n], th[j], acc);
        Out.p[j][n] = acc;
    }
}

__global__ __launch_bounds__(256) void k_pca_scale(Panel P, Factors f, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) P.p[blockIdx.y][i] *= f.v[blockIdx.y];
}

__global__ __launch_bounds__(64) void k_pca_decide(const double* __restrict__ theta, const double* __restrict__ S, int LM, int k,
                                                    const int* __restrict__ flag, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t < k) {
        out[t] = theta[t];
        out[k + t] = sqrt(S[t * LM + t]);
    }
    if (t == 0) out[2 * k] = (double)*flag;
}

// the better of two candidates of the sign rule: larger magnitude, then lower index
__device__ inline bool amax_better(double a1, long long i1, double a0, long long i0) { return a1 > a0 || (a1 == a0 && i1 < i0); }

__device__ inline void amax_reduce(double* sa, double* sv, long long* si, int t) {
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s && amax_better(sa[t + s], si[t + s], sa[t], si[t])) {
            sa[t] = sa[t + s];
            sv[t] = sv[t + s];
            si[t] = si[t + s];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_pca_amax(Panel U, int64_t npad, double* __restrict__ pv, long long* __restrict__ pi) {
    __shared__ double sa[256], sv[256];
    __shared__ long long si[256];
    const int t = threadIdx.x, j = blockIdx.y;
    double best = 0.0, bv = 0.0;
    long long bi = npad;
    for (int64_t n = (int64_t)blockIdx.x * 256 + t; n < npad; n += (int64_t)gridDim.x * 256) {
        const double v = U.p[j][n], a = fabs(v);
        if (a > best) { best = a; bv = v; bi = n; }
    }
    sa[t] = best; sv[t] = bv; si[t] = bi;
    __syncthreads();
    amax_reduce(sa, sv, si, t);
    if (t == 0) {
        pv[j * AMAX_BLOCKS + blockIdx.x] = sv[0];
        pi[j * AMAX_BLOCKS + blockIdx.x] = si[0];
    }
}

__global__ __launch_bounds__(256) void k_pca_emit(Panel U, Panel Out, int64_t npad, int nb, const double* __restrict__ pv,
                                                   const long long* __restrict__ pi) {
    __shared__ double sa[256], sv[256];
    __shared__ long long si[256];
    const int t = threadIdx.x, j = blockIdx.y;
    const double v0 = t < nb ? pv[j * AMAX_BLOCKS + t] : 0.0;
    sa[t] = fabs(v0); sv[t] = v0; si[t] = t < nb ? pi[j * AMAX_BLOCKS + t] : (long long)npad;
    __syncthreads();
    amax_reduce(sa, sv, si, t);
    const bool flip = sv[0] < 0.0;
    const int64_t n = (int64_t)blockIdx.x * 256 + t;
    if (n >= npad) return;
    const double v = U.p[j][n];
    Out.p[j][n] = v == 0.0 ? 0.0 : (flip ? -v : v);
}

// ---- scratch: owned by the context, grown on demand, freed with the dataset --------------------------------------------------------
struct Work {
    double *Q, *Y, *U, *R, *B;          // four N-space panels of L columns, one M-space panel
    double *part, *S, *W, *theta, *amax_v;
    long long* amax_i;
    int* flag;
    size_t bytes;
};

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

Work carve(char* base, int L, int64_t npad, int64_t mcap) {
    Work w{};
    size_t off = 0;
    auto take = [&](size_t nbytes) { char* p = base ? base + off : nullptr; off += up256(nbytes); return p; };
    const size_t pn = sizeof(double) * (size_t)L * (size_t)npad;
    w.Q = (double*)take(pn); w.Y = (double*)take(pn); w.U = (double*)take(pn); w.R = (double*)take(pn);
    w.B = (double*)take(sizeof(double) * (size_t)L * (size_t)mcap);
    w.part = (double*)take(sizeof(double) * GRAM_BLOCKS * LMAX * LMAX);
    w.S = (double*)take(sizeof(double) * LMAX * LMAX);
    w.W = (double*)take(sizeof(double) * LMAX * LMAX);
    w.theta = (double*)take(sizeof(double) * LMAX);
    w.amax_v = (double*)take(sizeof(double) * LMAX * AMAX_BLOCKS);
    w.amax_i = (long long*)take(sizeof(long long) * LMAX * AMAX_BLOCKS);
    w.flag = (int*)take(sizeof(int));
    w.bytes = off;
    return w;
}

// doubles between two columns of the M-space panel: every column starts on a 256-byte boundary, as a gv_vec does
inline int64_t m_stride(const gv_ctx* c) { return ((c->M > 0 ? c->M : 1) + 31) / 32 * 32; }

int reserve(gv_ctx* c, const char* who, int L, Work& w) {
    const int64_t mcap = m_stride(c);
    const size_t need = carve(nullptr, L, c->npad, mcap).bytes;
    if (!c->pca_scratch.reserve(need))
        return fail(c, "%s: cannot allocate %zu bytes of scratch (four N-space panels and one M-space panel of %d columns)", who, need, L);
    w = carve(static_cast<char*>(c->pca_scratch.buf), L, c->npad, mcap);
    return 0;
}

Panel panel_of(double* base, int L, int64_t stride) {
    Panel p{};
    for (int j = 0; j < L; j++) p.p[j] = base + (size_t)j * (size_t)stride;
    return p;
}

// S = X^T Y of two panels (LM x LM, zero beyond L)
void gram(gv_ctx* c, const Work& w, const Panel& X, const Panel& Y, int L) {
    const int64_t chunks = (c->npad + GRAM_ROWS - 1) / GRAM_ROWS;
    const int nb = gram_blocks(c->npad);
    const int64_t per = (chunks + nb - 1) / nb;
    const int LM = L <= 16 ? 16 : 32;
    if (LM == 16) hipLaunchKernelGGL(k_pca_gram<1>, dim3(nb), dim3(256), 0, c->stream, X, Y, L, c->npad, chunks, per, w.part);
    else hipLaunchKernelGGL(k_pca_gram<2>, dim3(nb), dim3(256), 0, c->stream, X, Y, L, c->npad, chunks, per, w.part);
    hipLaunchKernelGGL(k_pca_gram_fin, dim3(nblk(LM * LM, 32)), dim3(1024), 0, c->stream, w.part, nb, LM * LM, w.S);
}

void apply(gv_ctx* c, const Work& w, const Panel& X, int L, int Lout, const Panel* sub, const Panel& Out) {
    const int nb = nblk(c->npad, 256);
    const Panel& sb = sub ? *sub : X;
    if (L <= 16) hipLaunchKernelGGL(k_pca_apply<16>, dim3(nb), dim3(256), 0, c->stream, X, w.W, L, Lout, sb, w.theta, sub ? 1 : 0, Out, c->npad);
    else hipLaunchKernelGGL(k_pca_apply<32>, dim3(nb), dim3(256), 0, c->stream, X, w.W, L, Lout, sb, w.theta, sub ? 1 : 0, Out, c->npad);
}

// X <- orth(X): CholeskyQR applied twice, in place
void orth(gv_ctx* c, const Work& w, const Panel& X, int L) {
    const int LM = L <= 16 ? 16 : 32;
    for (int rep = 0; rep < 2; rep++) {
        gram(c, w, X, X, L);
        hipLaunchKernelGGL(k_pca_small, dim3(1), dim3(64), 0, c->stream, 0, w.S, L, LM, w.W, w.theta, w.flag);
        apply(c, w, X, L, L, nullptr, X);
    }
}

struct Events {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // products: 0 -> 1, Rayleigh-Ritz and residual: 1 -> 2, orth: 3 -> 4
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

double elapsed_s(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? 1e-3 * ms : 0.0;
}

const char* const CHOL_MSG =
    "gv_pca_dev: a Cholesky pivot is not positive (not above 32 * 2^-52 of its diagonal entry of the block's Gram matrix): the starting block "
    "is rank deficient to working precision, or the relationship matrix has rank below the block";

}  // namespace

namespace gvi {

// ---- the panel helpers for the other files that work on panels (gv_internal.h; gv_screen_cov.hip): the launches above, unchanged ----
size_t panel_bufs_bytes() {
    return up256(sizeof(double) * GRAM_BLOCKS * LMAX * LMAX) + 2 * up256(sizeof(double) * LMAX * LMAX) + up256(sizeof(double) * LMAX) +
           up256(sizeof(int));
}

PanelBufs panel_bufs_carve(char* base) {
    PanelBufs b{};
    size_t off = 0;
    auto take = [&](size_t nbytes) { char* p = base + off; off += up256(nbytes); return p; };
    b.part = (double*)take(sizeof(double) * GRAM_BLOCKS * LMAX * LMAX);
    b.S = (double*)take(sizeof(double) * LMAX * LMAX);
    b.W = (double*)take(sizeof(double) * LMAX * LMAX);
    b.theta = (double*)take(sizeof(double) * LMAX);
    b.flag = (int*)take(sizeof(int));
    return b;
}

static Work work_of(const PanelBufs& b) {
    Work w{};
    w.part = b.part; w.S = b.S; w.W = b.W; w.theta = b.theta; w.flag = b.flag;
    return w;
}

static Panel panel_from(double* const* p, int L) {
    Panel P{};
    for (int j = 0; j < L; j++) P.p[j] = p[j];
    return P;
}

void panel_gram(gv_ctx* c, const PanelBufs& b, double* const* X, double* const* Y, int L) {
    gram(c, work_of(b), panel_from(X, L), panel_from(Y, L), L);
}

void panel_orth(gv_ctx* c, const PanelBufs& b, double* const* X, int L) { orth(c, work_of(b), panel_from(X, L), L); }

// a k-array of handles of one space, all of this context and distinct; `seen` carries the vectors already named by the call
static int pca_handles(gv_ctx* c, const char* who, const char* arg, int n, const gv_vec* const* v, int space, bool outputs,
                       std::unordered_set<const gv_vec*>& seen) {
    for (int j = 0; j < n; j++) {
        if (!v[j]) return fail(c, "%s: the handle %s[%d] is NULL", who, arg, j);
        const std::string w = std::string(who) + ": column " + std::to_string(j);
        if (vec_need(c, w.c_str(), arg, v[j], space)) return 1;
        if (outputs && !seen.insert(v[j]).second) return fail(c, "%s: column %d: two outputs are the same vector", who, j);
    }
    return 0;
}

}  // namespace gvi

extern "C" {

int gv_pca_dev(gv_ctx* c, int k, int L, const gv_vec* const* q0, double tol, int max_iter, gv_vec* const* u, double* eval, double* resid) {
    if (!c) return 1;
    const char* who = "gv_pca_dev";
    NEED(c, k >= 1, "gv_pca_dev: k must be at least 1");
    NEED(c, L >= k, "gv_pca_dev: the block L must be at least k");
    if (L > LMAX) return fail(c, "gv_pca_dev: the block L = %d is above GV_PCA_MAX_BLOCK = %d", L, LMAX);
    NEED(c, tol > 0.0 && std::isfinite(tol), "gv_pca_dev: tol must be a positive finite number");
    NEED(c, max_iter >= 1, "gv_pca_dev: max_iter must be at least 1");
    NEED(c, q0 && u && eval && resid, "gv_pca_dev: q0, u, eval or resid is NULL");
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    std::unordered_set<const gv_vec*> outs;
    if (pca_handles(c, who, "u", k, u, GV_SPACE_N, true, outs)) return 1;
    if (pca_handles(c, who, "q0", L, q0, GV_SPACE_N, false, outs)) return 1;
    for (int j = 0; j < L; j++)
        if (outs.count(q0[j])) return fail(c, "gv_pca_dev: column %d: an output is also an input", j);
    const bool dense = c->dense.resident;
    NEED(c, c->have_stats && c->mask2, dense ? "Ax: methylation data, mask and marker statistics must be set first"
                                             : "Ax: bed, mask and marker statistics must be set first");
    const int64_t rank_max = c->nonas < c->Mt ? c->nonas : c->Mt;
    if (L > rank_max)
        return fail(c, "gv_pca_dev: the block L = %d is above min(nonas, Mt) = %lld, the most the rank of the relationship matrix can be", L,
                    (long long)rank_max);

    const auto t_call = std::chrono::steady_clock::now();
    Work w;
    if (reserve(c, who, L, w)) return 1;
    Events ev;
    for (hipEvent_t& x : ev.e) HIPCHK(c, hipEventCreate(&x));
    gv_pca_stats st{};
    st.block = L;
    st.scratch_bytes = w.bytes;
    hipStream_t s = c->stream;
    const int64_t npad = c->npad, mcap = m_stride(c);
    const int LM = L <= 16 ? 16 : 32;
    Panel Q = panel_of(w.Q, L, npad), Y = panel_of(w.Y, L, npad);
    const Panel U = panel_of(w.U, L, npad), R = panel_of(w.R, L, npad), B = panel_of(w.B, L, mcap);

    // Q <- orth(mask Q0), exact zeros at NA and pad slots
    HIPCHK(c, hipMemsetAsync(w.flag, 0, sizeof(int), s));
    HIPCHK(c, hipEventRecord(ev.e[3], s));
    for (int j = 0; j < L; j++) {
        gvk::mask_copy(s, Q.p[j], q0[j]->d, c->mask2, npad);
        if (npad > c->N) HIPCHK(c, hipMemsetAsync(Q.p[j] + c->N, 0, sizeof(double) * (size_t)(npad - c->N), s));
    }
    orth(c, w, Q, L);
    KCHK(c);
    HIPCHK(c, hipEventRecord(ev.e[4], s));

    Factors fy{};
    for (int j = 0; j < L; j++) fy.v[j] = (double)c->N / (double)c->Mt;
    std::vector<double> sc((size_t)(2 * k + 1));
    bool converged = false;
    int it = 0;
    while (true) {
        it++;
        HIPCHK(c, hipEventRecord(ev.e[0], s));
        if (atxm_device(c, L, Q.p, B.p)) return 1;                       // B = A^T Q
        if (score_device(c, L, B.p, Y.p)) return 1;                      // Y = (N / Mt) A B
        hipLaunchKernelGGL(k_pca_scale, dim3(nblk(npad, 256), L), dim3(256), 0, s, Y, fy, npad);
        HIPCHK(c, hipEventRecord(ev.e[1], s));
        gram(c, w, Q, Y, L);                                             // T = sym(Q^T Y) = V Theta V^T
        hipLaunchKernelGGL(k_pca_small, dim3(1), dim3(64), 0, s, 1, w.S, L, LM, w.W, w.theta, w.flag);
        apply(c, w, Q, L, L, nullptr, U);                                // U = Q V
        apply(c, w, Y, L, k, &U, R);                                     // R = Y V - U Theta, the first k columns
        gram(c, w, R, R, k);
        hipLaunchKernelGGL(k_pca_decide, dim3(1), dim3(64), 0, s, w.theta, w.S, k <= 16 ? 16 : 32, k, w.flag, c->red_out);
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e[2], s));
        if (read_scalars(c, 2 * k + 1, sc.data())) return 1;             // the one read-back of the iteration
        HIPCHK(c, hipEventSynchronize(ev.e[2]));
        st.seconds_products += elapsed_s(ev.e[0], ev.e[1]);
        st.seconds_panel += elapsed_s(ev.e[1], ev.e[2]) + elapsed_s(ev.e[3], ev.e[4]);
        st.cols_atxm += L;
        st.cols_score += L;
        if (sc[(size_t)(2 * k)] != 0.0) return fail(c, "%s", CHOL_MSG);
        converged = true;
        for (int i = 0; i < k; i++) converged = converged && sc[(size_t)(k + i)] <= tol * sc[(size_t)i];
        if (converged || it >= max_iter) break;
        HIPCHK(c, hipEventRecord(ev.e[3], s));
        orth(c, w, Y, L);                                                // Q <- orth(Y)
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e[4], s));
        std::swap(Q, Y);
    }

    // the sign rule on the first k columns of U, into the caller's vectors
    const int ab = nblk(npad, 256) < AMAX_BLOCKS ? nblk(npad, 256) : AMAX_BLOCKS;
    Panel out{};
    for (int j = 0; j < k; j++) out.p[j] = u[j]->d;
    hipLaunchKernelGGL(k_pca_amax, dim3(ab, k), dim3(256), 0, s, U, npad, w.amax_v, w.amax_i);
    hipLaunchKernelGGL(k_pca_emit, dim3(nblk(npad, 256), k), dim3(256), 0, s, U, out, npad, ab, w.amax_v, w.amax_i);
    KCHK(c);
    for (int i = 0; i < k; i++) {
        eval[i] = sc[(size_t)i];
        resid[i] = sc[(size_t)(k + i)];
    }
    st.iterations = it;
    st.converged = converged ? 1 : 0;
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count();
    c->pca_last = st;
    return 0;
}

int gv_pca_loadings_dev(gv_ctx* c, int k, const gv_vec* const* u, const double* eval, gv_vec* const* v) {
    if (!c) return 1;
    const char* who = "gv_pca_loadings_dev";
    NEED(c, k >= 1, "gv_pca_loadings_dev: k must be at least 1");
    if (k > LMAX) return fail(c, "gv_pca_loadings_dev: k = %d is above GV_PCA_MAX_BLOCK = %d", k, LMAX);
    NEED(c, u && eval && v, "gv_pca_loadings_dev: u, eval or v is NULL");
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    std::unordered_set<const gv_vec*> outs;
    if (pca_handles(c, who, "v", k, v, GV_SPACE_M, true, outs)) return 1;
    if (pca_handles(c, who, "u", k, u, GV_SPACE_N, false, outs)) return 1;
    Factors f{};
    Panel P{}, O{};
    const double rn = sqrt((double)c->N / (double)c->Mt);
    for (int i = 0; i < k; i++) {
        if (!(eval[i] > 0.0) || !std::isfinite(eval[i])) return fail(c, "gv_pca_loadings_dev: eval[%d] is not a positive finite number", i);
        f.v[i] = rn / sqrt(eval[i]);
        P.p[i] = u[i]->d;
        O.p[i] = v[i]->d;
    }
    if (atxm_device(c, k, P.p, O.p)) return 1;
    if (c->M > 0) hipLaunchKernelGGL(k_pca_scale, dim3(nblk(c->M, 256), k), dim3(256), 0, c->stream, O, f, c->M);
    KCHK(c);
    return 0;
}

int gv_pca_info(const gv_ctx* c, gv_pca_stats* out) {
    if (!c || !out) return 1;
    *out = c->pca_last;
    return 0;
}

}  // extern "C"
