// Flow likelihood (diffusion.FlowLikelihood): the log-density of the eta = 0 DDIM sampler's model by the
// change of variables along the ascending (encoding) walk.  Three kernels around the engine's frozen forward and full
// backward: the Rademacher probe handed to the backward as deps, the step that turns the backward's dx into the trace
// estimate, the log-determinant term and the encode update, and the closing prior term.  None allocates, none
// synchronises, the position is read from the device.
#include <math.h>

#include "cdm_common.h"
#include "cdm_hip.h"
#include "sampler_parts.h"

namespace cdm {

// v of element e (within the map) at the position p: +1 where u < 0.5, else -1, u element e of the stream
// cdm_philox_uniform(out, H H, 0, 1, key, sub = p) writes.  Keyed by position and element, not by the row.
static __device__ __forceinline__ float probe_elem(unsigned long long key, int p, long long e) {
    return philox_u01_elem(key, (uint32_t)p, e) < 0.5f ? 1.f : -1.f;
}

static __device__ __forceinline__ unsigned long long probe_key(unsigned long long seed, const long long* seed_dev) {
    return run_key(seed, seed_dev) ^ FLOW_PROBE_DOMAIN;
}

__global__ void flow_probe_kernel(float* v, int n, long long HW, const int* cur_k, int npos, unsigned long long seed,
                                  const long long* seed_dev) {
    const int p = *cur_k;
    if (p < 1 || p > npos) return;
    const unsigned long long key = probe_key(seed, seed_dev);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < HW; e += (long long)gridDim.x * blockDim.x) {
        const float s = probe_elem(key, p, e);
        for (int b = 0; b < n; ++b) v[(long long)b * HW + e] = s;
    }
}

// The block's fp64 sum, valid in thread 0: per-thread partials, a wave64 butterfly, then (w0 + w1) + (w2 + w3) through
// LDS (obs_residual_grad_kernel's order).  Every thread of the 256 must call it.
static __device__ __forceinline__ double block_sum_d(double acc, double* red) {
#pragma clang fp contract(off)
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// log(1 + a) for a > -1 from IEEE operations alone (+, -, *, /, frexp; every line one fp64 rounding, nothing fused), so
// that a host restatement gives the same bits whatever its libm:
//   y = 1 + a;  (m, e) = frexp(y), m doubled and e lowered by one where m < sqrt(1/2): y = m 2^e, m in [sqrt(1/2), sqrt 2)
//   s = a / (2 + a)  where e == 0 (no rounding of 1 + a enters: small a keeps its relative accuracy)
//   s = (m - 1) / (m + 1)  otherwise;        |s| <= 0.1716
//   log(1 + a) = e ln2 + 2 s (1 + z/3 + z^2/5 + ... + z^11/23),  z = s^2, by Horner from the last term
// The truncation error is below 2e-20 relative to the series; a few ulp of rounding.
static __device__ __forceinline__ double log1p_ieee(double a) {
#pragma clang fp contract(off)
    const double y = 1.0 + a;
    int e;
    double m = frexp(y, &e);
    if (m < 0.70710678118654752440) { m = m * 2.0; e -= 1; }
    const double s = e == 0 ? a / (2.0 + a) : (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double h = 1.0 / 23.0;
#pragma unroll
    for (int k = 21; k >= 1; k -= 2) h = h * z + 1.0 / (double)k;
    const double r = (2.0 * s) * h;
    return (double)e * 0.69314718055994530942 + r;
}

// One block of 256 threads per row.  At the position p = *cur_k, with v regenerated from its key (the buffer the
// backward was handed is not trusted to be intact):
//   q       = sum_e (double)dx[e] (double)v[e]     fp64: thread t adds e = t, t + 256, ... ascending, block_sum_d
//   FORM 0 (trace):   ld = g[p] q
//   FORM 1 (logdet):  a = (g[p] q) / D;  ld = D log1p_ieee(a) where a > -1, else NaN      (D = H H)
//   acc[row] += ld;  hist[p n + row] = q;  invalid[row] = 1 where ld is not finite (never cleared here)
//   x[e] <- ix[p] x[e] + ie[p] eps[e]             fp32, two products and one sum, each one rounding
template <int FORM>
__global__ __launch_bounds__(256) void flow_step_kernel(float* x, const float* eps, const float* dx, int n, long long HW,
                                                        const int* cur_k, const float* ix, const float* ie,
                                                        const double* g, int npos, unsigned long long seed,
                                                        const long long* seed_dev, double* acc, double* hist,
                                                        int* invalid) {
#pragma clang fp contract(off)  // separate roundings, as the restatement computes them
    const int p = *cur_k;
    if (p < 1 || p > npos) return;                      // block-uniform
    const int row = blockIdx.x;
    const long long base = (long long)row * HW;
    const unsigned long long key = probe_key(seed, seed_dev);
    const float a = ix[p], c = ie[p];
    double part = 0.0;
    for (long long e = threadIdx.x; e < HW; e += 256) {
        part = part + (double)dx[base + e] * (double)probe_elem(key, p, e);
        x[base + e] = a * x[base + e] + c * eps[base + e];
    }
    __shared__ double red[4];
    const double q = block_sum_d(part, red);
    if (threadIdx.x == 0) {
        const double gq = g[p] * q, D = (double)HW;
        double ld;
        if (FORM == 0) ld = gq;
        else {
            const double r = gq / D;
            ld = r > -1.0 ? D * log1p_ieee(r) : (double)NAN;
        }
        acc[row] = acc[row] + ld;
        hist[(long long)p * n + row] = q;
        if (!isfinite(ld)) invalid[row] = 1;
    }
}

// Per row: ss = sum_e (double)x[e] (double)x[e] in flow_step_kernel's order, prior = -0.5 ss - (0.5 D) log(2 pi),
// logp = (prior + (0.5 D) log_abT) + acc[row], each line one fp64 rounding.
__global__ __launch_bounds__(256) void flow_finish_kernel(const float* x, long long HW, double log_abT, const double* acc,
                                                          double* prior, double* logp) {
#pragma clang fp contract(off)
    const int row = blockIdx.x;
    const long long base = (long long)row * HW;
    double part = 0.0;
    for (long long e = threadIdx.x; e < HW; e += 256) {
        const double xe = (double)x[base + e];
        part = part + xe * xe;
    }
    __shared__ double red[4];
    const double ss = block_sum_d(part, red);
    if (threadIdx.x == 0) {
        const double hD = 0.5 * (double)HW;
        const double pr = -0.5 * ss - hD * 1.83787706640934548356;   // log(2 pi)
        prior[row] = pr;
        logp[row] = (pr + hD * log_abT) + acc[row];
    }
}

}  // namespace cdm

using namespace cdm;
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

CDM_API int cdm_flow_probe(float* v, int n, int H, const int* cur_k, int npos, unsigned long long seed,
                           const long long* seed_dev, void* stream) {
    if (!v || !cur_k || n < 1 || H < 1 || npos < 1) return (int)hipErrorInvalidValue;
    const long long HW = (long long)H * H;
    hipLaunchKernelGGL(flow_probe_kernel, dim3(nblocks(HW)), dim3(256), 0, S(stream), v, n, HW, cur_k, npos, seed,
                       seed_dev);
    return cdm_status();
}

CDM_API int cdm_flow_step(float* x, const float* eps, const float* dx, int n, int H, const int* cur_k, const float* ix,
                          const float* ie, const double* g, int npos, int form, unsigned long long seed,
                          const long long* seed_dev, double* acc, double* hist, int* invalid, void* stream) {
    if (!x || !eps || !dx || !cur_k || !ix || !ie || !g || !acc || !hist || !invalid || n < 1 || H < 1 || npos < 1 ||
        (form != 0 && form != 1))
        return (int)hipErrorInvalidValue;
    const long long HW = (long long)H * H;
    if (form == 0)
        hipLaunchKernelGGL(flow_step_kernel<0>, dim3(n), dim3(256), 0, S(stream), x, eps, dx, n, HW, cur_k, ix, ie, g,
                           npos, seed, seed_dev, acc, hist, invalid);
    else
        hipLaunchKernelGGL(flow_step_kernel<1>, dim3(n), dim3(256), 0, S(stream), x, eps, dx, n, HW, cur_k, ix, ie, g,
                           npos, seed, seed_dev, acc, hist, invalid);
    return cdm_status();
}

CDM_API int cdm_flow_finish(const float* x, int n, int H, double log_abT, const double* acc, double* prior, double* logp,
                            void* stream) {
    if (!x || !acc || !prior || !logp || n < 1 || H < 1 || !(log_abT <= 0.0) || !(log_abT > -INFINITY))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_finish_kernel, dim3(n), dim3(256), 0, S(stream), x, (long long)H * H, log_abT, acc, prior,
                       logp);
    return cdm_status();
}
