// gv_dense_fx.h -- device functions the epilogues of the fixed-point dosage route share (gv_dense_mfma.hip: k_dm_fin_atx, k_dm_fin_ax;
// gv_dense_atxm.hip: k_dm_fin_atxm).  One copy, so that a column of the batch product is rounded by the very expression the one-vector
// product runs: contraction cannot separate them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gvdm {

// the pass's one integer sum_k q_k = hi 2^32 + lo from the block limb sums (every block of an epilogue for itself; integers: any order)
__device__ inline void limb_total(const long long* __restrict__ limb, int nb, long long& hi, long long& lo) {
    __shared__ long long sh[2][256];
    long long h = 0, l = 0;
    for (int b = threadIdx.x; b < nb; b += 256) { h += limb[2 * b]; l += limb[2 * b + 1]; }
    sh[0][threadIdx.x] = h;
    sh[1][threadIdx.x] = l;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh[0][threadIdx.x] += sh[0][threadIdx.x + off]; sh[1][threadIdx.x] += sh[1][threadIdx.x + off]; }
        __syncthreads();
    }
    hi = sh[0][0];
    lo = sh[1][0];
}
// hi 2^32 + lo with 0 <= lo < 2^32 after the carry: (double)hi 2^32 and (double)lo are exact (|hi| < 2^53), their sum rounds once
__device__ inline double limbs_to_double(long long hi, long long lo) {
    hi += lo >> 32;
    lo &= 0xFFFFFFFFLL;
    return fma((double)hi, 4294967296.0, (double)lo);
}
// the seven digit planes of one row over the K-segments: value = hi 2^32 + lo (exact, as combine() of gv_mfma.hip).  A row of a partial
// plane holds `width` int32 columns, the seven planes wanted start at column `col`
__device__ inline void gather(const int32_t* __restrict__ part, int segs, int64_t rows_p, int64_t row, int width, int col, long long& hi,
                              long long& lo) {
    long long s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < segs; k++) {
        const int4* q = reinterpret_cast<const int4*>(part + ((int64_t)k * rows_p + row) * width + col);
        const int4 x0 = q[0], x1 = q[1];
        s[0] += x0.x; s[1] += x0.y; s[2] += x0.z; s[3] += x0.w;
        s[4] += x1.x; s[5] += x1.y; s[6] += x1.z;
    }
    lo = s[0] + (s[1] << 8) + (s[2] << 16) + (s[3] << 24);
    hi = s[4] + (s[5] << 8) + (s[6] << 16);
}
// ATx of one marker and vector: msig scale_x (S1 - (mu' - 128) Q) 2^(e-54) scale from the integers S1 = (sh, sl) and Q = (qh, ql)
__device__ inline double atx_value(double dmu, double msig, double wscale, double scale, double scal, long long qh, long long ql,
                                   long long sh, long long sl) {
    const double core = fma(-(dmu - 128.0), limbs_to_double(qh, ql), limbs_to_double(sh, sl));
    return (msig * wscale) * (core * scal) * scale;
}

}  // namespace gvdm
