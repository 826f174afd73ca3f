// Probe: v_mfma_f64_16x16x4_f64 on gfx950 -- its lane maps, checked with exact integer data, and its issue rate: a bare loop with the
// operands in registers and 4 independent accumulators per wave, one workgroup per CU, at one and at two waves per SIMD, on random
// data.  The rate is the yardstick of the GRM block kernel.  Prints one JSON line.
//   hipcc --offload-arch=gfx950 -O3 -o scripts/probes/mfma_f64_rate scripts/probes/mfma_f64_rate.hip && scripts/probes/mfma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double v4d __attribute__((ext_vector_type(4)));

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            printf("%s failed: %s\n", #x, hipGetErrorString(e_));                          \
            return 2;                                                                      \
        }                                                                                  \
    } while (0)

__global__ void k_layout(const double* a, const double* b, v4d* d) {
    const int l = threadIdx.x;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[l], b[l], acc, 0, 0, 0);
    d[l] = acc;
}

// every wave: iters x 4 MFMAs on 4 accumulators that do not depend on each other
__global__ void k_rate(const double* in, double* out, int iters) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const double a0 = in[2 * t], b0 = in[2 * t + 1];
    const double a1 = a0 * 0.5, b1 = b0 * 0.25;
    v4d c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    for (int i = 0; i < iters; i++) {
        c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c3, 0, 0, 0);
    }
    const v4d s = c0 + c1 + c2 + c3;
    out[t] = s[0] + s[1] + s[2] + s[3];
}

int main() {
    // 1. the lane maps: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D: col = l & 15, row = (l >> 4) + 4 reg
    double A[16][4], B[4][16], D[16][16];
    srand(1);
    for (int r = 0; r < 16; r++)
        for (int k = 0; k < 4; k++) A[r][k] = rand() % 7 - 3;
    for (int k = 0; k < 4; k++)
        for (int c = 0; c < 16; c++) B[k][c] = rand() % 255 - 127;      // (asymmetric: a transposed C-write does not pass)
    for (int r = 0; r < 16; r++)
        for (int c = 0; c < 16; c++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += A[r][k] * B[k][c];
            D[r][c] = s;
        }
    double ha[64], hb[64], hd[64][4];
    for (int l = 0; l < 64; l++) {
        ha[l] = A[l & 15][l >> 4];
        hb[l] = B[l >> 4][l & 15];
    }
    double *da, *db;
    v4d* dd;
    CK(hipMalloc(&da, sizeof(ha)));
    CK(hipMalloc(&db, sizeof(hb)));
    CK(hipMalloc(&dd, sizeof(hd)));
    CK(hipMemcpy(da, ha, sizeof(ha), hipMemcpyHostToDevice));
    CK(hipMemcpy(db, hb, sizeof(hb), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, da, db, dd);
    CK(hipMemcpy(hd, dd, sizeof(hd), hipMemcpyDeviceToHost));
    int bad = 0, bad_f32 = 0;
    for (int l = 0; l < 64; l++)
        for (int reg = 0; reg < 4; reg++) {
            bad += hd[l][reg] != D[(l >> 4) + 4 * reg][l & 15];
            bad_f32 += hd[l][reg] != D[4 * (l >> 4) + reg][l & 15];
        }
    if (bad) {
        printf("{\"layout_mismatches\": %d, \"f32_row_formula_mismatches\": %d}\n", bad, bad_f32);
        return 1;
    }
    // 2. the rate
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, iters = 100000;
    const size_t nthr = (size_t)cus * 512;
    std::vector<double> hin(2 * nthr);
    for (double& v : hin) v = (double)rand() / RAND_MAX - 0.5;
    double *din, *dout;
    CK(hipMalloc(&din, sizeof(double) * hin.size()));
    CK(hipMalloc(&dout, sizeof(double) * nthr));
    CK(hipMemcpy(din, hin.data(), sizeof(double) * hin.size(), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    double rate[2] = {0, 0};
    for (int w = 0; w < 2; w++) {           // 256 threads = 1 wave per SIMD, 512 = 2
        const int threads = 256 << w;
        double best = 1e30;
        for (int rep = 0; rep < 4; rep++) {          // (the first one warms up)
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(k_rate, dim3(cus), dim3(threads), 0, 0, din, dout, iters);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        rate[w] = (double)cus * (threads / 64) * (double)iters * 4.0 * 1024.0 / (best * 1e-3);
    }
    printf("{\"instruction\": \"v_mfma_f64_16x16x4_f64\", \"layout_mismatches\": 0, \"f32_row_formula_mismatches\": %d, \"cus\": %d, "
           "\"clock_mhz\": %d, \"iters\": %d, \"accumulators\": 4, \"macs_per_s_1_wave_per_simd\": %.6e, \"macs_per_s_2_waves_per_simd\": %.6e}\n",
           bad_f32, cus, prop.clockRate / 1000, iters, rate[0], rate[1]);
    return 0;
}
