// Parameter fit (likelihood.ParamFit): gradient descent on the scan score over the conditioning vector.
// Three small kernels around the engine's frozen forward and truncated backward: the objective's value and gradient
// at the network output, the fp64 accumulation of dc over positions, and the fp64 Adam update with its bookkeeping.
// None allocates, none synchronises, every index (timestep, pass) is read from the device.
#include "cdm_common.h"
#include "cdm_hip.h"

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

static __device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One block per row m K + k.  d = pred - noise in fp32; deps = coef * d (one fp32 product), coef = the fp32 rounding of
// (2 w[i] inv_R) / HW formed in fp64; acc[m ld + k0 + k] += (((double)w[i] * sum d^2) / HW) * inv_R.
// Element order of a row: `head` scalar elements up to the first 16-byte boundary of the pred row, then float4 groups,
// then a scalar tail.  pred and deps rows share their offset, so both are aligned on the body when their base
// addresses agree mod 16 (otherwise the whole row is scalar); the noise row has its own offset (m HW, not row HW)
// and is read as a float4 only where it is aligned too.  Thread t owns head element t, groups t, t + 256, ... and tail
// element t: a fixed element set per thread, then scan_mse_accum_kernel's butterfly and fold — the same bits every run.
__global__ __launch_bounds__(256) void fit_mse_grad_kernel(const float* pred, const float* noise, int K, int HW, int T,
                                                           const int* cur_i, const float* w, double inv_R, double* acc,
                                                           int ld, int k0, float* deps) {
    const int i = *cur_i;
    if (i < 1 || i > T) return;                         // block-uniform
    const int row = blockIdx.x, m = row / K, k = row - m * K;
    const float* pr = pred + (long long)row * HW;
    const float* nz = noise + (long long)m * HW;
    float* dp = deps + (long long)row * HW;
    const double wi = (double)w[i];
    const float coef = (float)(((2.0 * wi) * inv_R) / (double)HW);
    const uintptr_t ap = reinterpret_cast<uintptr_t>(pr), ad = reinterpret_cast<uintptr_t>(dp);
    const bool vec = ((ap ^ ad) & 15) == 0;             // no common alignment: the whole row goes through the tail loop
    int head = vec ? (int)(((16 - (ap & 15)) & 15) >> 2) : 0;
    if (head > HW) head = HW;
    const int nvec = vec ? (HW - head) >> 2 : 0, tail0 = head + 4 * nvec;
    const bool nz4 = (reinterpret_cast<uintptr_t>(nz + head) & 15) == 0;
    double s = 0.0;
    if ((int)threadIdx.x < head) {
        const int e = threadIdx.x;
        const float d = pr[e] - nz[e];
        dp[e] = coef * d;
        s = fma((double)d, (double)d, s);               // the product is exact in fp64: fma == multiply, then add
    }
    for (int g = threadIdx.x; g < nvec; g += 256) {
        const int e = head + 4 * g;
        const float4 a = ld4(pr + e);
        const float4 b = nz4 ? ld4(nz + e) : make_float4(nz[e], nz[e + 1], nz[e + 2], nz[e + 3]);
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
        st4(dp + e, make_float4(coef * d0, coef * d1, coef * d2, coef * d3));
        s = fma((double)d0, (double)d0, s);
        s = fma((double)d1, (double)d1, s);
        s = fma((double)d2, (double)d2, s);
        s = fma((double)d3, (double)d3, s);
    }
    for (int e = tail0 + threadIdx.x; e < HW; e += 256) {
        const float d = pr[e] - nz[e];
        dp[e] = coef * d;
        s = fma((double)d, (double)d, s);
    }
    __shared__ double red[4];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        const double term = ((wi * tot) / (double)HW) * inv_R;
        acc[(long long)m * ld + k0 + k] = acc[(long long)m * ld + k0 + k] + term;
    }
}

__global__ void fit_grad_accum_kernel(const float* dc, long long n, double* gacc) {
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x)
        gacc[q] += (double)dc[q];
}

// One block, rows taken in tiles of 256.  Per tile: the per-row part, one thread per row (the gradient norm over the
// free columns, the finite and better flags into LDS, history, stall count); a barrier; then one thread per (row,
// column) of the tile for best_c and the Adam step.  Both read only values from before the pass.  After the last tile
// phase 2 folds the score into best_score, clears the accumulators and counters for the next pass and advances the
// pass index — so no thread reads what another writes.
__global__ __launch_bounds__(256) void fit_update_kernel(int* done, int iters, int rows, int ncf, double* score,
                                                         double* gacc, const int* free_mask, const double* lo,
                                                         const double* hi, double lr, double beta1, double beta2,
                                                         double eps, const double* bc, double* c64, float* c32, double* m,
                                                         double* v, double* best_score, float* best_c, double* hist_score,
                                                         double* hist_gnorm, int* stalled, int* pos_ctr) {
#pragma clang fp contract(off)  // plain IEEE fp64: one rounding per operation, in the order written
    const int n0 = *done;                               // passes completed so far; this is pass n = n0 + 1
    if (n0 < 0 || n0 > iters) return;                   // block-uniform: past the last pass nothing is touched
    const bool update = n0 < iters;
    const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
    const double bc1 = update ? bc[2 * n0] : 1.0, bc2 = update ? bc[2 * n0 + 1] : 1.0;
    const int total = rows * ncf;
    __shared__ unsigned char row_finite[256], row_better[256];
    for (int row0 = 0; row0 < rows; row0 += 256) {      // block-uniform trip count
        const int nrow = rows - row0 < 256 ? rows - row0 : 256;
        if ((int)threadIdx.x < nrow) {
            const int row = row0 + threadIdx.x;
            const double sc = score[row];
            double ss = 0.0;
            bool finite = isfinite(sc);
            for (int j = 0; j < ncf; ++j) {
                if (!free_mask[j]) continue;
                const double gj = gacc[row * ncf + j];
                finite = finite && isfinite(gj);
                ss = ss + gj * gj;
            }
            hist_score[(long long)n0 * rows + row] = sc;
            hist_gnorm[(long long)n0 * rows + row] = sqrt(ss);
            if (update && !finite) stalled[row] += 1;
            row_finite[threadIdx.x] = finite;
            row_better[threadIdx.x] = sc < best_score[row];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nrow * ncf; e += 256) {
            const int r = e / ncf, j = e - r * ncf, q = row0 * ncf + e;
            if (row_better[r]) best_c[q] = c32[q];
            if (!update || !row_finite[r] || !free_mask[j]) continue;
            const double g = gacc[q];
            const double m1 = beta1 * m[q] + omb1 * g;
            const double v1 = beta2 * v[q] + omb2 * (g * g);
            const double mhat = m1 / bc1, vhat = v1 / bc2;
            const double step = (lr * mhat) / (sqrt(vhat) + eps);
            double c = c64[q] - step;
            c = c < lo[j] ? lo[j] : (c > hi[j] ? hi[j] : c);
            m[q] = m1; v[q] = v1; c64[q] = c; c32[q] = (float)c;
        }
        __syncthreads();                                // the next tile rewrites the flags
    }
    for (int q = threadIdx.x; q < total; q += blockDim.x) gacc[q] = 0.0;
    for (int row = threadIdx.x; row < rows; row += blockDim.x) {
        const double sc = score[row];
        if (sc < best_score[row]) best_score[row] = sc;
        score[row] = 0.0;
    }
    if (threadIdx.x == 0) { *done = n0 + 1; if (pos_ctr) *pos_ctr = 0; }
}

CDM_API int cdm_fit_mse_grad(const float* pred, const float* noise, int M, int K, int HW, const int* cur_i,
                             const float* w, int T, double inv_R, double* acc, int ld, int k0, float* deps,
                             void* stream) {
    if (!pred || !noise || !cur_i || !w || !acc || !deps || M < 1 || K < 1 || HW < 1 || T < 1 || k0 < 0 ||
        ld < k0 + K || (long long)M * K > 0x7fffffffLL || !(inv_R > 0.0))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fit_mse_grad_kernel, dim3(M * K), dim3(256), 0, S(stream), pred, noise, K, HW, T, cur_i, w, inv_R,
                       acc, ld, k0, deps);
    return cdm_status();
}

CDM_API int cdm_fit_grad_accum(const float* dc, int rows, int ncf, double* gacc, void* stream) {
    if (!dc || !gacc || rows < 1 || ncf < 1) return (int)hipErrorInvalidValue;
    const long long n = (long long)rows * ncf;
    const int nb = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(fit_grad_accum_kernel, dim3(nb), dim3(256), 0, S(stream), dc, n, gacc);
    return cdm_status();
}

CDM_API int cdm_fit_update(int* done, int iters, int rows, int ncf, double* score, double* gacc, const int* free_mask,
                           const double* lo, const double* hi, double lr, double beta1, double beta2, double eps,
                           const double* bc, double* c64, float* c32, double* m, double* v, double* best_score,
                           float* best_c, double* hist_score, double* hist_gnorm, int* stalled, int* pos_ctr,
                           void* stream) {
    if (!done || !score || !gacc || !free_mask || !lo || !hi || !bc || !c64 || !c32 || !m || !v || !best_score ||
        !best_c || !hist_score || !hist_gnorm || !stalled || iters < 1 || rows < 1 || ncf < 1 ||
        (long long)rows * ncf > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fit_update_kernel, dim3(1), dim3(256), 0, S(stream), done, iters, rows, ncf, score, gacc,
                       free_mask, lo, hi, lr, beta1, beta2, eps, bc, c64, c32, m, v, best_score, best_c, hist_score,
                       hist_gnorm, stalled, pos_ctr);
    return cdm_status();
}
