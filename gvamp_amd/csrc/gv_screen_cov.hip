// gv_screen_cov.hip -- the covariate-adjusted association screen: gv_screen_cov_set, gv_screen_cov_dev,
// gv_screen_cov_info.  The regression of every phenotype column on [1, covariates, g_j] for every marker j by partial regression
// (Frisch-Waugh-Lovell): the batch product (gv_atxm.hip) is called as it is, on the orthonormal basis Q of the covariates once per set
// and on the unit-norm residuals of the phenotypes once per call; this file is everything around those two products.  A panel is
// L <= 32 separate fp64 columns of npad doubles (gv_pca.hip), whose Gram and CholeskyQR kernels are reused through gvi::panel_gram /
// gvi::panel_orth.  No atomics; every sum in an order that is a function of npad alone.
//
//   k_cov_mask         column blockIdx.y of the caller's vectors into the work panel, exact zeros outside the mask (NA and pad slots)
//   k_cov_sum<SQ>      per column the sum (SQ = 0: s += v) or the sum of squares (SQ = 1: s = fma(v, v, s)) of all npad slots: a
//                      grid-stride loop of sum_blocks(npad) blocks of 256 threads, each thread's terms in index order, the block's 256
//                      sums in a fixed tree; k_cov_sum_fin: the block partials of a column in the same tree
//   k_cov_centre       q <- q - fl(sum / n) at the phenotyped individuals
//   k_cov_unit         q <- fl(q / fl(sqrt(ss)))
//   k_cov_project<KM>  y[n] <- fma(-q_k[n], g_kj, y[n]) for k ascending, g = Q^T Y from k_pca_gram; one thread per row, the row of Q in
//                      registers; KM = 16 or 32 by K alone, so a column's arithmetic does not depend on the other columns
//   k_cov_v            v_j = fma(-c, sum_k z_jk^2, 1) from the M x K panel
//   k_screen_cov_fin   the five outputs per marker and column (gvamp.h: the rounding sequence)
#include <chrono>
#include <cmath>
#include <cstring>

#include "gv_internal.h"
#include "gv_pval_dev.h"

using namespace gvi;

namespace {

constexpr int LMAX = GV_PCA_MAX_BLOCK;
constexpr int SUM_BLOCKS = 256;        // most blocks per column of a sum (= the threads that add their partials)

struct Panel { double* p[LMAX]; };
struct InCols { const double* p[LMAX]; };
struct FinCols { double* r[LMAX]; double* t[LMAX]; double* p[LMAX]; double* beta[LMAX]; double* se[LMAX]; };

inline int nblk(int64_t n, int per) { return (int)((n + per - 1) / per); }
inline int sum_blocks(int64_t npad) {
    const int64_t b = (npad + 255) / 256;
    return (int)(b < 1 ? 1 : (b > SUM_BLOCKS ? SUM_BLOCKS : b));
}
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

__device__ inline bool present(const uint32_t* __restrict__ mask2, int64_t n) { return (mask2[n >> 4] >> (2 * (n & 15))) & 1u; }

__global__ __launch_bounds__(256) void k_cov_mask(InCols in, Panel out, const uint32_t* __restrict__ mask2, int64_t npad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    out.p[blockIdx.y][n] = present(mask2, n) ? in.p[blockIdx.y][n] : 0.0;
}

__device__ inline double block_tree(double* sm, int t) {
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sm[t] += sm[t + s];
        __syncthreads();
    }
    return sm[0];
}

template <int SQ>
__global__ __launch_bounds__(256) void k_cov_sum(Panel P, int64_t npad, double* __restrict__ part) {
    __shared__ double sm[256];
    const int t = threadIdx.x;
    const double* __restrict__ p = P.p[blockIdx.y];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < npad; i += (int64_t)gridDim.x * 256) {
        const double v = p[i];
        s = SQ ? fma(v, v, s) : s + v;
    }
    sm[t] = s;
    __syncthreads();
    const double tot = block_tree(sm, t);
    if (t == 0) part[blockIdx.y * SUM_BLOCKS + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_cov_sum_fin(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double sm[256];
    const int t = threadIdx.x;
    sm[t] = t < nb ? part[blockIdx.x * SUM_BLOCKS + t] : 0.0;
    __syncthreads();
    const double tot = block_tree(sm, t);
    if (t == 0) out[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_cov_centre(Panel P, const double* __restrict__ sums, double n_phen, const uint32_t* __restrict__ mask2,
                                                     int64_t npad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    const double mean = sums[blockIdx.y] / n_phen;
    double* p = P.p[blockIdx.y];
    p[n] = present(mask2, n) ? p[n] - mean : 0.0;
}

__global__ __launch_bounds__(256) void k_cov_unit(Panel P, const double* __restrict__ ss, int64_t npad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    double* p = P.p[blockIdx.y];
    p[n] = p[n] / sqrt(ss[blockIdx.y]);
}

// G = Q^T Y: K x nc entries of the LM x LM row-major matrix k_pca_gram_fin left
template <int KM>
__global__ __launch_bounds__(256) void k_cov_project(Panel Q, int K, Panel Y, int nc, const double* __restrict__ G, int LM, int64_t npad) {
    __shared__ double g[KM * LMAX];
    for (int e = threadIdx.x; e < KM * LMAX; e += 256) {
        const int i = e / LMAX, j = e % LMAX;
        g[e] = (i < K && j < nc) ? G[i * LM + j] : 0.0;
    }
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    double q[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) q[i] = i < K ? Q.p[i][n] : 0.0;
    for (int j = 0; j < nc; j++) {
        double acc = Y.p[j][n];
#pragma unroll
        for (int i = 0; i < KM; i++) acc = fma(-q[i], g[i * LMAX + j], acc);
        Y.p[j][n] = acc;
    }
}

__global__ __launch_bounds__(256) void k_cov_v(Panel Z, int K, double c, int64_t M, double* __restrict__ v) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double s = 0.0;
    for (int k = 0; k < K; k++) {
        const double z = Z.p[k][m];
        s = fma(z, z, s);
    }
    v[m] = fma(-c, s, 1.0);
}

__global__ __launch_bounds__(256) void k_screen_cov_fin(FinCols a, int64_t M, const uint32_t* __restrict__ cnt, const double* __restrict__ mave,
                                                         const double* __restrict__ msig, const double* __restrict__ qss, double wscale2,
                                                         const double* __restrict__ v, const double* __restrict__ ss, double afac, double nu,
                                                         double nm1, double vif_max) {
    const int c = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    // the variance input.  Bed data: sumsqx of gvp::marker_stats, in its expression (k_screen_fin's rule), sxx = (n - 1) / msig^2.
    // Dosage codes (qss != NULL, gv_set_screen_dosage): q of the statistics pass, sxx = scale^2 q
    const double sg = msig[m];
    double sumsqx, sxx;
    if (qss) {
        sumsqx = qss[m];
        sxx = wscale2 * sumsqx;
    } else {
        const double n2 = cnt[3 * m], n1 = cnt[3 * m + 1], n0 = cnt[3 * m + 2], mu = mave[m];
        sumsqx = sg * sg * (n2 * (2.0 - mu) * (2.0 - mu) + n1 * (1.0 - mu) * (1.0 - mu) + n0 * mu * mu);
        sxx = nm1 / (sg * sg);
    }
    const double vj = v[m], S = ss[c];
    double r, t, p, beta, se;
    r = t = p = beta = se = NAN;
    if (sumsqx != 0.0 && !(vj * vif_max < 1.0) && S > 0.0) {
        const double rho = (a.r[c][m] * afac) / sqrt(vj);
        if (!isnan(rho)) {
            const double om = fma(-rho, rho, 1.0);
            const double d = sxx * vj;
            r = rho;
            beta = rho * sqrt(S / d);
            if (om <= 0.0) {
                t = copysign(__longlong_as_double(0x7ff0000000000000LL), rho);
                p = 0.0;
                se = 0.0;
            } else {
                t = rho * sqrt(nu / om);
                p = gvp::t_two_sided(fabs(t), nu);
                se = sqrt((S * om) / (nu * d));
            }
        }
    }
    a.r[c][m] = r;
    if (a.t[c]) a.t[c][m] = t;
    if (a.p[c]) a.p[c][m] = p;
    if (a.beta[c]) a.beta[c][m] = beta;
    if (a.se[c]) a.se[c][m] = se;
}

// ---- the work panels, in the context's pca_scratch: the small buffers of the panel kernels, L N-space columns, a column of zeros (the
// columns of a Gram beyond a panel's own), Lm M-space columns and one more for v, the block partials and the results of the sums
struct Work {
    PanelBufs b;
    double *A, *zero, *B, *v, *part, *sums, *ss;
    size_t bytes;
};

inline int64_t m_stride(const gv_ctx* c) { return ((c->M > 0 ? c->M : 1) + 31) / 32 * 32; }

Work carve(char* base, int L, int Lm, int64_t npad, int64_t mcap) {
    Work w{};
    size_t off = 0;
    auto take = [&](size_t nbytes) { char* p = base ? base + off : nullptr; off += up256(nbytes); return p; };
    char* pb = take(panel_bufs_bytes());
    if (base) w.b = panel_bufs_carve(pb);
    w.A = (double*)take(sizeof(double) * (size_t)(L > 0 ? L : 1) * (size_t)npad);
    w.zero = (double*)take(sizeof(double) * (size_t)npad);
    w.B = (double*)take(sizeof(double) * (size_t)(Lm > 0 ? Lm : 1) * (size_t)mcap);
    w.v = (double*)take(sizeof(double) * (size_t)mcap);
    w.part = (double*)take(sizeof(double) * LMAX * SUM_BLOCKS);
    w.sums = (double*)take(sizeof(double) * LMAX);
    w.ss = (double*)take(sizeof(double) * LMAX);
    w.bytes = off;
    return w;
}

int reserve(gv_ctx* c, const char* who, int L, int Lm, Work& w) {
    const int64_t mcap = m_stride(c);
    const size_t need = carve(nullptr, L, Lm, c->npad, mcap).bytes;
    if (!c->pca_scratch.reserve(need)) return fail(c, "%s: cannot allocate %zu bytes of scratch (the work panels of %d columns)", who, need, L);
    w = carve(static_cast<char*>(c->pca_scratch.buf), L, Lm, c->npad, mcap);
    return 0;
}

// the columns of `in` into the panel, masked and centred over the phenotyped: w.sums is left holding the masked sums
void mask_centre(gv_ctx* c, const Work& w, const InCols& in, const Panel& P, int L) {
    hipStream_t s = c->stream;
    const int nb = nblk(c->npad, 256), sb = sum_blocks(c->npad);
    hipLaunchKernelGGL(k_cov_mask, dim3(nb, L), dim3(256), 0, s, in, P, c->mask2, c->npad);
    hipLaunchKernelGGL(k_cov_sum<0>, dim3(sb, L), dim3(256), 0, s, P, c->npad, w.part);
    hipLaunchKernelGGL(k_cov_sum_fin, dim3(L), dim3(256), 0, s, w.part, sb, w.sums);
    hipLaunchKernelGGL(k_cov_centre, dim3(nb, L), dim3(256), 0, s, P, w.sums, (double)c->nonas, c->mask2, c->npad);
}

// w.ss = the columns' sums of squares; P <- P / sqrt(ss)
void unit_norm(gv_ctx* c, const Work& w, const Panel& P, int L) {
    hipStream_t s = c->stream;
    const int nb = nblk(c->npad, 256), sb = sum_blocks(c->npad);
    hipLaunchKernelGGL(k_cov_sum<1>, dim3(sb, L), dim3(256), 0, s, P, c->npad, w.part);
    hipLaunchKernelGGL(k_cov_sum_fin, dim3(L), dim3(256), 0, s, w.part, sb, w.ss);
    hipLaunchKernelGGL(k_cov_unit, dim3(nb, L), dim3(256), 0, s, P, w.ss, c->npad);
}

struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

double elapsed_s(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? 1e-3 * ms : 0.0;
}

// what both entry points need of the context: the state gv_screen_dev asks for, under the caller's name
int need_screen_state(gv_ctx* c, const char* who) {
    const bool dosage = screen_dosage(c);      // gv_set_screen_dosage is on and dosage codes are resident
    if (c->dense.resident && !dosage) return fail(c, "%s: no screen is defined for methylation or dosage data (2-bit genotypes only)", who);
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    NEED(c, c->have_stats && c->mask2 && (dosage ? c->dense.qss != nullptr : c->counts != nullptr),
         "ATx: bed and marker statistics must be set first");
    if (c->alpha_scale != 1.0) return fail(c, "%s: the marker statistics must be those of alpha_scale = 1 (r is a correlation)", who);
    if (c->nonas < 3) return fail(c, "%s: fewer than 3 individuals with a phenotype leave the test no degree of freedom", who);
    return 0;
}

const char* const COLLINEAR = "the covariates are collinear with each other or with the intercept";

}  // namespace

extern "C" {

int gv_screen_cov_set(gv_ctx* c, int K, const gv_vec* const* cov) {
    if (!c) return 1;
    const char* who = "gv_screen_cov_set";
    if (K < 0 || K > LMAX) return fail(c, "gv_screen_cov_set: K = %d covariates, outside 0 .. GV_PCA_MAX_BLOCK = %d", K, LMAX);
    NEED(c, K == 0 || cov, "gv_screen_cov_set: the array of covariate handles is NULL");
    if (need_screen_state(c, who)) return 1;
    const int64_t nu = c->nonas - 2 - K;
    if (nu < 1)
        return fail(c, "gv_screen_cov_set: %lld phenotyped individuals and %d covariates leave nu = n - 2 - K = %lld degrees of freedom (at least 1)",
                    (long long)c->nonas, K, (long long)nu);
    for (int k = 0; k < K; k++) {
        if (!cov[k]) return fail(c, "gv_screen_cov_set: the handle cov[%d] is NULL", k);
        const std::string w = std::string(who) + ": column " + std::to_string(k);
        if (vec_need(c, w.c_str(), "cov", cov[k], GV_SPACE_N)) return 1;
    }

    const auto t_call = std::chrono::steady_clock::now();
    Work w;
    if (reserve(c, who, K, K, w)) return 1;
    Events ev;
    for (hipEvent_t& x : ev.e) HIPCHK(c, hipEventCreate(&x));
    hipStream_t s = c->stream;
    const int64_t npad = c->npad, mcap = m_stride(c), M = c->M;
    Panel Q{}, Z{};
    InCols in{};
    for (int k = 0; k < K; k++) {
        Q.p[k] = w.A + (size_t)k * (size_t)npad;
        Z.p[k] = w.B + (size_t)k * (size_t)mcap;
        in.p[k] = cov[k]->d;
    }
    HIPCHK(c, hipEventRecord(ev.e[0], s));
    if (K > 0) {
        HIPCHK(c, hipMemsetAsync(w.b.flag, 0, sizeof(int), s));
        mask_centre(c, w, in, Q, K);
        unit_norm(c, w, Q, K);
        panel_orth(c, w.b, Q.p, K);
        KCHK(c);
    }
    HIPCHK(c, hipEventRecord(ev.e[1], s));
    if (K > 0) {
        // the one read-back of the call: the sums of squares and the Cholesky flag decide whether the covariates are usable
        std::vector<double> ss((size_t)K);
        int flag = 0;
        HIPCHK(c, hipMemcpyAsync(ss.data(), w.ss, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&flag, w.b.flag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int k = 0; k < K; k++)
            if (!(ss[(size_t)k] > 0.0) || !std::isfinite(ss[(size_t)k]))
                return fail(c, "gv_screen_cov_set: covariate %d is constant over the phenotyped individuals or not finite there: %s", k, COLLINEAR);
        if (flag)
            return fail(c, "gv_screen_cov_set: a Cholesky pivot is not positive (not above 32 * 2^-52 of its diagonal entry of the covariates' Gram "
                           "matrix): %s", COLLINEAR);
        if (atxm_device(c, K, Q.p, Z.p)) return 1;
    }
    HIPCHK(c, hipEventRecord(ev.e[2], s));
    if (M > 0) hipLaunchKernelGGL(k_cov_v, dim3(nblk(M, 256)), dim3(256), 0, s, Z, K, (double)c->N / (double)(c->nonas - 1), M, w.v);
    KCHK(c);
    // nothing can refuse from here on but the allocation of the cache, and a cache that had to grow holds nothing
    const size_t qbytes = up256(sizeof(double) * (size_t)K * (size_t)npad), vbytes = sizeof(double) * (size_t)mcap;
    if (qbytes + vbytes > c->cov_cache.cap) cov_drop(c);
    if (!c->cov_cache.reserve(qbytes + vbytes)) {
        cov_drop(c);
        return fail(c, "gv_screen_cov_set: cannot allocate %zu bytes for the cached basis and v", qbytes + vbytes);
    }
    char* cache = static_cast<char*>(c->cov_cache.buf);
    if (K > 0) HIPCHK(c, hipMemcpyAsync(cache, w.A, sizeof(double) * (size_t)K * (size_t)npad, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(cache + qbytes, w.v, sizeof(double) * (size_t)(M > 0 ? M : 0), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(ev.e[3], s));
    HIPCHK(c, hipEventSynchronize(ev.e[3]));
    c->have_cov = true;
    c->cov_K = K;
    gv_screen_cov_stats& st = c->cov_last;
    st.set_seconds_products = elapsed_s(ev.e[1], ev.e[2]);
    st.set_seconds_panel = elapsed_s(ev.e[0], ev.e[1]) + elapsed_s(ev.e[2], ev.e[3]);
    st.set_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count();
    return 0;
}

int gv_screen_cov_dev(gv_ctx* c, int64_t C, const gv_vec* const* y, double vif_max, gv_vec* const* r, gv_vec* const* t, gv_vec* const* p,
                      gv_vec* const* beta, gv_vec* const* se) {
    if (!c) return 1;
    const char* who = "gv_screen_cov_dev";
    NEED(c, C >= 0, "gv_screen_cov_dev: the number of columns is negative");
    NEED(c, std::isfinite(vif_max) && vif_max >= 1.0, "gv_screen_cov_dev: vif_max must be a finite number, at least 1");
    if (need_screen_state(c, who)) return 1;
    NEED(c, c->have_cov, "gv_screen_cov_dev: gv_screen_cov_set must be called first (after the last gv_set_mask, gv_marker_stats or upload: "
                         "the cached covariate basis belongs to the mask and marker statistics it was computed from)");
    if (C == 0) return 0;
    NEED(c, y && r, "gv_screen_cov_dev: the arrays of column handles are NULL");
    std::vector<const double*> ys;
    std::vector<double*> rs;
    if (batch_args(c, who, C, y, r, "y", GV_SPACE_N, ys, rs)) return 1;
    // t, p, beta, se: M-space vectors of this context, distinct from each other, from r and from the inputs
    std::unordered_set<const gv_vec*> seen;
    for (int64_t j = 0; j < C; j++) { seen.insert(y[j]); seen.insert(r[j]); }
    gv_vec* const* const opt[4] = {t, p, beta, se};
    const char* const opt_name[4] = {"t", "p", "beta", "se"};
    for (int a = 0; a < 4; a++) {
        if (!opt[a]) continue;
        for (int64_t j = 0; j < C; j++) {
            if (!opt[a][j]) return fail(c, "gv_screen_cov_dev: the handle of column %lld is NULL", (long long)j);
            const std::string w = "gv_screen_cov_dev: column " + std::to_string((long long)j);
            if (vec_need(c, w.c_str(), opt_name[a], opt[a][j], GV_SPACE_M)) return 1;
            if (!seen.insert(opt[a][j]).second) return fail(c, "gv_screen_cov_dev: column %lld: two outputs are the same vector", (long long)j);
        }
    }

    const auto t_call = std::chrono::steady_clock::now();
    const int K = c->cov_K;
    const int Lw = (int)(C < LMAX ? C : LMAX);
    Work w;
    if (reserve(c, who, Lw, 0, w)) return 1;
    Events ev;
    for (hipEvent_t& x : ev.e) HIPCHK(c, hipEventCreate(&x));
    hipStream_t s = c->stream;
    const int64_t npad = c->npad, M = c->M;
    const size_t qbytes = up256(sizeof(double) * (size_t)K * (size_t)npad);
    double* const cq = static_cast<double*>(c->cov_cache.buf);
    const double* const cv = reinterpret_cast<const double*>(static_cast<char*>(c->cov_cache.buf) + qbytes);
    const double afac = sqrt((double)c->N / (double)(c->nonas - 1)), nu = (double)(c->nonas - 2 - K), nm1 = (double)(c->nonas - 1);
    gv_screen_cov_stats st = c->cov_last;
    st.columns = C;
    st.call_seconds_products = st.call_seconds_panel = 0.0;
    HIPCHK(c, hipMemsetAsync(w.zero, 0, sizeof(double) * (size_t)npad, s));
    for (int64_t j0 = 0; j0 < C; j0 += LMAX) {
        const int nc = (int)(C - j0 < LMAX ? C - j0 : LMAX);
        const int L = K > nc ? K : nc;                   // the Gram's panels: both padded with the column of zeros to L columns
        Panel Y{}, Qg{}, Yg{};
        InCols in{};
        FinCols fc{};
        for (int j = 0; j < L; j++) {
            Qg.p[j] = j < K ? cq + (size_t)j * (size_t)npad : w.zero;
            Yg.p[j] = j < nc ? w.A + (size_t)j * (size_t)npad : w.zero;
        }
        for (int j = 0; j < nc; j++) {
            Y.p[j] = w.A + (size_t)j * (size_t)npad;
            in.p[j] = ys[(size_t)(j0 + j)];
            fc.r[j] = rs[(size_t)(j0 + j)];
            fc.t[j] = t ? t[j0 + j]->d : nullptr;
            fc.p[j] = p ? p[j0 + j]->d : nullptr;
            fc.beta[j] = beta ? beta[j0 + j]->d : nullptr;
            fc.se[j] = se ? se[j0 + j]->d : nullptr;
        }
        HIPCHK(c, hipEventRecord(ev.e[0], s));
        mask_centre(c, w, in, Y, nc);
        for (int rep = 0; rep < 2 && K > 0; rep++) {
            panel_gram(c, w.b, Qg.p, Yg.p, L);
            const int LM = L <= 16 ? 16 : 32, nb = nblk(npad, 256);
            if (K <= 16) hipLaunchKernelGGL(k_cov_project<16>, dim3(nb), dim3(256), 0, s, Qg, K, Y, nc, w.b.S, LM, npad);
            else hipLaunchKernelGGL(k_cov_project<32>, dim3(nb), dim3(256), 0, s, Qg, K, Y, nc, w.b.S, LM, npad);
        }
        unit_norm(c, w, Y, nc);
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e[1], s));
        if (atxm_device(c, nc, Y.p, fc.r)) return 1;
        HIPCHK(c, hipEventRecord(ev.e[2], s));
        if (M > 0)
            hipLaunchKernelGGL(k_screen_cov_fin, dim3(nblk(M, 256), nc), dim3(256), 0, s, fc, M, c->counts, c->mave, c->msig,
                               screen_dosage(c) ? c->dense.qss : nullptr, c->dense.scale * c->dense.scale, cv, w.ss, afac, nu, nm1, vif_max);
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e[3], s));
        HIPCHK(c, hipEventSynchronize(ev.e[3]));         // (the four events are the next block's)
        st.call_seconds_products += elapsed_s(ev.e[1], ev.e[2]);
        st.call_seconds_panel += elapsed_s(ev.e[0], ev.e[1]) + elapsed_s(ev.e[2], ev.e[3]);
    }
    st.call_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count();
    c->cov_last = st;
    return 0;
}

int gv_screen_cov_info(const gv_ctx* c, gv_screen_cov_stats* out) {
    if (!c || !out) return 1;
    *out = c->cov_last;
    out->K = c->have_cov ? c->cov_K : -1;
    out->pad_ = 0;
    out->nu = c->have_cov ? c->nonas - 2 - c->cov_K : 0;
    out->cached_bytes = c->have_cov ? up256(sizeof(double) * (size_t)c->cov_K * (size_t)c->npad) + sizeof(double) * (size_t)m_stride(c) : 0;
    return 0;
}

}  // extern "C"
