// gv_precond.hip -- the LD-block preconditioner of the M-space CG solves (gv_set_cg_precond kind 1).
//
// Windows of W markers on GLOBAL marker indices, two grids staggered by h = W/2: window u >= 0 covers [(u-1)h, (u+1)h), clipped
// to [0, Mt) and to the shard [S, S+M).  Odd u is grid 0 (window k = (u-1)/2 = [kW, kW+W)), even u is grid 1 (window k = u/2 =
// [kW-h, kW+h), the first one clipped at 0).  Every marker lies in exactly one window of each grid: u = g/h and g/h + 1.
//   Gram      G_u = the window's exact diagonal block of A^T A, from the resident 2-bit re-encoding with i8 MFMA: the Gram epilogue of
//             k_ld_block (gvp::gram, gv_ld.hip); of resident 8-bit dosage codes under gv_set_ld_dosage: the Gram epilogue of k_ldd_block
//             (gvp::gram_dosage; section 18)
//   factor    B_u = tau G_u + gam2 I, Cholesky in LDS and the explicit inverse L^-T L^-1, one workgroup per window (k_pc_factor)
//   apply     z = 1/2 sum over both grids of blockdiag(B_u^-1) r (k_pc_apply)
// Integer Grams, then a fixed fp64 order everywhere, no atomics: the results do not depend on the layout or the launch.
#include <chrono>
#include <cmath>

#include "gv_internal.h"

namespace {

// one workgroup per window: B = tau G + gam2 I in LDS, Cholesky B = L L^T (L strictly below the diagonal of a, its diagonal in dl),
// X = L^-1 by column-wise forward substitution (X^T on and above the diagonal of a), then B^-1 = X^T X -- symmetric and positive
// definite by construction.  A pivot <= 1e-12 x the window's largest diagonal, or not finite, sends the window to the scalar rule.
__global__ __launch_bounds__(256) void k_pc_factor(const double* __restrict__ gram, int W, int64_t S, int64_t M, int64_t u0, double tau,
                                                   double gam2, double diag, double* __restrict__ inv, int* __restrict__ fail) {
    extern __shared__ double a[];            // W * W, then the diagonal of L
    double* dl = a + W * W;
    __shared__ double dmax_s;
    __shared__ int bad_s;
    const int H = W / 2;
    const int64_t u = u0 + blockIdx.x;
    const int n = (int)(min((u + 1) * H, S + M) - max((u - 1) * H, S));
    const double* G = gram + (int64_t)blockIdx.x * W * W;
    for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
        const int i = e / n, j = e % n;
        a[i * W + j] = tau * G[(int64_t)i * W + j] + (i == j ? gam2 : 0.0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int i = 0; i < n; i++) m = fmax(m, a[i * W + i]);
        dmax_s = m;
        bad_s = 0;
    }
    __syncthreads();
    const double thr = 1e-12 * dmax_s;
    for (int k = 0; k < n; k++) {            // right-looking Cholesky on the lower triangle
        const double p = a[k * W + k];       // (every thread reads the same pivot: the exit is uniform)
        if (!(p > thr) || !isfinite(p)) {
            if (threadIdx.x == 0) bad_s = 1;
            break;
        }
        const double l = sqrt(p);
        if (threadIdx.x == 0) dl[k] = l;
        for (int i = k + 1 + threadIdx.x; i < n; i += blockDim.x) a[i * W + k] /= l;
        __syncthreads();
        const int m = n - k - 1;
        for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) a[i * W + j] -= a[i * W + k] * a[j * W + k];
        }
        __syncthreads();
    }
    __syncthreads();
    const bool bad = bad_s != 0;
    if (!bad)
        for (int j = threadIdx.x; j < n; j += blockDim.x) {     // column j of X = L^-1, stored as row j of a from the diagonal on
            a[j * W + j] = 1.0 / dl[j];
            for (int i = j + 1; i < n; i++) {
                double s = 0.0;
                for (int k = j; k < i; k++) s = fma(a[i * W + k], a[j * W + k], s);
                a[j * W + i] = -s / dl[i];
            }
        }
    __syncthreads();
    double* out = inv + (int64_t)blockIdx.x * W * W;
    for (int e = threadIdx.x; e < W * W; e += blockDim.x) {
        const int i = e / W, j = e % W;
        double x = 0.0;
        if (i < n && j < n) {
            if (bad) x = i == j ? 1.0 / diag : 0.0;
            else                              // (X^T X)_ij = sum_{k >= max(i, j)} X_ki X_kj, the same order for (i, j) and (j, i)
                for (int k = max(i, j); k < n; k++) x = fma(a[i * W + k], a[j * W + k], x);
        }
        out[e] = x;
    }
    if (threadIdx.x == 0) fail[blockIdx.x] = bad ? 1 : 0;
}

// z[i] = 1/2 (B_ua^-1 r + B_ub^-1 r)[i] for local marker i, ua = g/h and ub = ua + 1 (g = S + i); fixed order
__global__ __launch_bounds__(256) void k_pc_apply(const double* __restrict__ inv, int W, int64_t S, int64_t M, int64_t u0,
                                                  const double* __restrict__ r, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int H = W / 2;
    const int64_t g = S + i;
    double s[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int64_t u = g / H + q;
        const int64_t lo = max((u - 1) * H, S) - S, len = min((u + 1) * H, S + M) - S - lo;
        const double* B = inv + (u - u0) * W * W + (i - lo);     // column i - lo = row i - lo (symmetric)
        double acc = 0.0;
        for (int64_t j = 0; j < len; j++) acc = fma(B[j * W], r[lo + j], acc);
        s[q] = acc;
    }
    z[i] = 0.5 * (s[0] + s[1]);
}

}  // namespace

namespace gvp {
int64_t first_window(int64_t S, int W) { return S / (W / 2); }
int64_t num_windows(int64_t S, int64_t M, int W) { return M > 0 ? (S + M - 1) / (W / 2) + 2 - S / (W / 2) : 0; }

size_t factor_lds(int W) { return sizeof(double) * ((size_t)W * W + W); }

int factor(hipStream_t s, const double* gram, int W, int64_t S, int64_t M, double tau, double gam2, double diag, double* inv, int* fail) {
    const int64_t u0 = first_window(S, W), nu = num_windows(S, M, W);
    if (nu == 0) return 0;
    const size_t lds = factor_lds(W);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pc_factor), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(k_pc_factor, dim3((unsigned)nu), dim3(256), lds, s, gram, W, S, M, u0, tau, gam2, diag, inv, fail);
    return 0;
}

void apply(hipStream_t s, const double* inv, int W, int64_t S, int64_t M, const double* r, double* z) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_pc_apply, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, inv, W, S, M, first_window(S, W), r, z);
}
}  // namespace gvp

// ---- the context side and the C ABI ----------------------------------------------------------------------------------------------
using namespace gvi;

namespace gvi {
void pc_invalidate(gv_ctx* c, bool free_mem) {
    c->pc_have_gram = c->pc_have_inv = false;
    if (!free_mem) return;
    for (void* p : {(void*)c->pc_gram, (void*)c->pc_inv, (void*)c->pc_fail})
        if (p) (void)hipFree(p);
    c->pc_gram = c->pc_inv = nullptr;
    c->pc_fail = nullptr;
    c->pc_nu = 0;
}

// the window Grams of the resident data set (once per data set, mask and marker statistics)
static int pc_build_gram(gv_ctx* c) {
    NEED(c, c->pc_kind == 1, "LD preconditioner: not enabled (gv_set_cg_precond(ctx, 1, window))");
    const bool codes = c->dense.resident && c->dense.bits;      // compact dosage data: the Gram epilogue of k_ldd_block, or a refusal
    if (codes ? gram_dosage_check(c, "LD preconditioner") : planes_check(c, "LD preconditioner", "genotype windows only")) return 1;
    const int W = c->pc_W;
    if (!c->pc_have_gram) {
        const int64_t u0 = gvp::first_window(c->S, W), nu = gvp::num_windows(c->S, c->M, W);
        if (nu != c->pc_nu || !c->pc_gram) {
            pc_invalidate(c, true);
            const size_t bytes = sizeof(double) * (size_t)(nu > 0 ? nu : 1) * W * W;
            HIPCHK(c, hipMalloc(&c->pc_gram, bytes));
            HIPCHK(c, hipMalloc(&c->pc_inv, bytes));
            HIPCHK(c, hipMalloc(&c->pc_fail, sizeof(int) * (size_t)(nu > 0 ? nu : 1)));
        }
        c->pc_u0 = u0;
        c->pc_nu = nu;
        const gvm::Plan& pl = c->plan;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const auto t0 = std::chrono::steady_clock::now();
        if (codes) {
            if (gvp::gram_dosage(c, c->pc_gram)) return 1;
        } else
            gvp::gram(c->stream, pl.layout == 1 ? pl.tiles : pl.stripes_m, pl.layout, pl.nkb_m, c->mask2, c->pitch / 4, c->N, c->S, c->M, W,
                      c->mave, c->msig, c->pc_gram);
        KCHK(c);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->pc_build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        c->pc_have_gram = true;
        c->pc_have_inv = false;
    }
    return 0;
}

int pc_prepare(gv_ctx* c, double tau, double gam2) {
    if (pc_build_gram(c)) return 1;
    const int W = c->pc_W;
    if (c->pc_have_inv && tau == c->pc_tau && gam2 == c->pc_gam2) return 0;
    const double diag = tau * (double)(c->N - 1) / (double)c->N + gam2;     // the scalar rule of a window that falls back
    if (gvp::factor(c->stream, c->pc_gram, W, c->S, c->M, tau, gam2, diag, c->pc_inv, c->pc_fail))
        return fail(c, "LD preconditioner: cannot give the factorisation kernel %zu bytes of LDS", sizeof(double) * ((size_t)W * W + W));
    KCHK(c);
    std::vector<int> fl((size_t)c->pc_nu);
    if (c->pc_nu > 0) HIPCHK(c, hipMemcpyAsync(fl.data(), c->pc_fail, sizeof(int) * fl.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t nf = 0;
    for (int f : fl) nf += f;
    c->pc_fallback = nf;
    c->pc_factorisations++;
    c->pc_tau = tau;
    c->pc_gam2 = gam2;
    c->pc_have_inv = true;
    return 0;
}

void pc_apply(gv_ctx* c, const double* r, double* z) { gvp::apply(c->stream, c->pc_inv, c->pc_W, c->S, c->M, r, z); }
}  // namespace gvi

extern "C" {

int gv_set_cg_precond(gv_ctx* c, int kind, int window) {
    NEED(c, kind == 0 || kind == 1, "gv_set_cg_precond: kind must be 0 (scalar, the default) or 1 (ld)");
    NEED(c, kind == 0 || window == 32 || window == 64 || window == 128, "gv_set_cg_precond: window must be 32, 64 or 128");
    // compact dosage data: accepted while gv_set_ld_dosage is on and the codes are 8 bits wide
    if (kind != 0 && ld_dosage(c)) {
        if (c->dense.bits != 8)
            return fail(c, "gv_set_cg_precond: gv_set_ld_dosage covers 8-bit codes only: the resident data are 16-bit codes (their hi / lo byte "
                           "split is not built)");
    } else if (kind != 0) {
        REFUSE_DOSAGE(c, "gv_set_cg_precond", "the LD preconditioner works on genotype windows only");
        NEED(c, !c->dense.resident, "gv_set_cg_precond: the LD preconditioner is refused for dense (meth) data");
    }
    if (kind == 0 || window != c->pc_W) pc_invalidate(c, true);     // (kind 0 releases the Grams and inverses)
    c->pc_kind = kind;
    if (kind == 1) c->pc_W = window;
    return 0;
}

int gv_precond_info(gv_ctx* c, gv_precond_stats* info) {
    NEED(c, info, "gv_precond_info: info is NULL");
    *info = gv_precond_stats{};
    info->kind = c->pc_kind;
    info->window = c->pc_W;
    const int64_t u0 = gvp::first_window(c->S, c->pc_W), nu = gvp::num_windows(c->S, c->M, c->pc_W);
    for (int64_t u = u0; u < u0 + nu; u++) {      // odd u: grid 0 window (u - 1) / 2; even u: grid 1 window u / 2
        const int grid = (u & 1) ? 0 : 1;
        const int64_t k = (u & 1) ? (u - 1) / 2 : u / 2;
        if (info->windows[grid]++ == 0) info->first_window[grid] = k;
    }
    info->resident_bytes = c->pc_gram ? 2.0 * sizeof(double) * (double)c->pc_nu * c->pc_W * c->pc_W : 0.0;
    info->build_seconds = c->pc_build_s;
    info->factorisations = c->pc_factorisations;
    info->fallback_windows = c->pc_fallback;
    info->last_tau = c->pc_tau;
    info->last_gam2 = c->pc_gam2;
    return 0;
}

int gv_precond_window_gram(gv_ctx* c, int grid, int64_t k, double* out) {
    NEED(c, grid == 0 || grid == 1, "gv_precond_window_gram: grid must be 0 or 1");
    NEED(c, c->pc_kind == 1, "gv_precond_window_gram: the LD preconditioner is not enabled");
    if (pc_build_gram(c)) return 1;         // (reading a Gram factorises nothing)
    const int64_t u = grid == 0 ? 2 * k + 1 : 2 * k;
    NEED(c, k >= 0 && u >= c->pc_u0 && u < c->pc_u0 + c->pc_nu, "gv_precond_window_gram: the window does not overlap this shard");
    const size_t n = (size_t)c->pc_W * c->pc_W;
    HIPCHK(c, hipMemcpyAsync(out, c->pc_gram + (size_t)(u - c->pc_u0) * n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gv_precond_apply(gv_ctx* c, double tau, double gam2, const gv_vec* r, gv_vec* z) {
    NEED(c, r && z && r->space == GV_SPACE_M && z->space == GV_SPACE_M && r != z, "gv_precond_apply: M-space r and z, no aliasing");
    NEED_VEC(c, "gv_precond_apply", r, GV_SPACE_M);
    NEED_VEC(c, "gv_precond_apply", z, GV_SPACE_M);
    if (pc_prepare(c, tau, gam2)) return 1;
    pc_apply(c, r->d, z->d);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
