// Timestep-aware training loss (Trainer(loss_weight=..., t_sampler=..., t_record=...)): the per-row MSE with
// a per-timestep weight and the importance weight of the draw, the per-bucket record of the raw loss, the loss-aware
// timestep table rebuilt from that record, and the draw that reads it.  None allocates, none synchronises, every
// table is read from the device, so the three sit inside the captured training step.
//
// Buckets: NB of them over 1..T, edge_k = (k T) / NB in integer arithmetic, bucket k = edge_k + 1 .. edge_{k+1};
// the bucket of a timestep t is (t NB - 1) / T.
#include "sampler_parts.h"
#include "cdm_hip.h"

using namespace cdm;
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

static __device__ __forceinline__ int tl_edge(int k, int T, int NB) { return (int)(((long long)k * T) / NB); }

// One thread per sample.  k = the count of j in 0..NB-2 with cdf[j] <= (double)u0 (cdf[NB - 1] is never read, so a
// u0 of exactly 1 lands in the last bucket); t uniform within the bucket from u1, clamped for the same reason.
__global__ void tsample_draw_kernel(int* t, float* iw, int B, int T, int NB, const double* cdf, const float* iw_tab,
                                    unsigned long long seed, uint32_t sub, const int* sub_dev) {
    if (sub_dev) sub += (uint32_t)*sub_dev;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        const float u0 = philox_u01_elem(seed, sub, 2ll * b), u1 = philox_u01_elem(seed, sub, 2ll * b + 1);
        const double u = (double)u0;
        int k = 0;
        for (int j = 0; j < NB - 1; ++j) k += cdf[j] <= u ? 1 : 0;
        const int e0 = tl_edge(k, T, NB), nk = tl_edge(k + 1, T, NB) - e0;
        t[b] = e0 + 1 + min(nk - 1, (int)((float)nk * u1));
        iw[b] = iw_tab[k];
    }
}

// omega_b = w_tab[t_b] * iw[b], one fp32 product; an absent table is 1
static __device__ __forceinline__ float tl_omega(const int* t, const float* w_tab, const float* iw, int b) {
    const float w = w_tab ? w_tab[t[b]] : 1.f, i = iw ? iw[b] : 1.f;
    return w * i;
}

// One block per row b.  d = pred - noise in fp32; dpred = d * (scale * omega_b), the factor one fp32 product (with both
// tables absent it is scale itself: mse_kernel's bits); row_sq[b] = sum d^2 and row_g[b] = sum dpred in fp64.
// Element order of a row: fit_mse_grad_kernel's (csrc/fit.hip): a scalar head up to the first 16-byte boundary of the
// pred row, float4 groups, a scalar tail; all three rows share their offset b HW, so the body is vectorised when the
// three base addresses agree mod 16, else the whole row is scalar.  Thread t owns head element t, groups t, t + 256,
// ... and tail element t; then a wave64 butterfly and a fixed-order fold of the four wave sums: the same bits every run.
__global__ __launch_bounds__(256) void mse_weighted_kernel(const float* pred, const float* noise, int HW, const int* t,
                                                           const float* w_tab, const float* iw, float scale,
                                                           float* dpred, double* row_sq, double* row_g) {
    const int b = blockIdx.x;
    const float* pr = pred + (long long)b * HW;
    const float* nz = noise + (long long)b * HW;
    float* dp = dpred + (long long)b * HW;
    const float coef = (w_tab || iw) ? scale * tl_omega(t, w_tab, iw, b) : scale;
    const uintptr_t ap = reinterpret_cast<uintptr_t>(pr), an = reinterpret_cast<uintptr_t>(nz),
                    ad = reinterpret_cast<uintptr_t>(dp);
    const bool vec = (((ap ^ ad) | (ap ^ an)) & 15) == 0;
    int head = vec ? (int)(((16 - (ap & 15)) & 15) >> 2) : 0;
    if (head > HW) head = HW;
    const int nvec = vec ? (HW - head) >> 2 : 0, tail0 = head + 4 * nvec;
    double s = 0.0, g = 0.0;
    if ((int)threadIdx.x < head) {
        const int e = threadIdx.x;
        const float d = pr[e] - nz[e], gd = d * coef;
        dp[e] = gd;
        s = fma((double)d, (double)d, s);               // the product is exact in fp64: fma == multiply, then add
        g += (double)gd;
    }
    for (int q = threadIdx.x; q < nvec; q += 256) {
        const int e = head + 4 * q;
        const float4 a = ld4(pr + e), n4 = ld4(nz + e);
        const float d0 = a.x - n4.x, d1 = a.y - n4.y, d2 = a.z - n4.z, d3 = a.w - n4.w;
        const float g0 = d0 * coef, g1 = d1 * coef, g2 = d2 * coef, g3 = d3 * coef;
        st4(dp + e, make_float4(g0, g1, g2, g3));
        s = fma((double)d0, (double)d0, s);
        s = fma((double)d1, (double)d1, s);
        s = fma((double)d2, (double)d2, s);
        s = fma((double)d3, (double)d3, s);
        g += (double)g0; g += (double)g1; g += (double)g2; g += (double)g3;
    }
    for (int e = tail0 + threadIdx.x; e < HW; e += 256) {
        const float d = pr[e] - nz[e], gd = d * coef;
        dp[e] = gd;
        s = fma((double)d, (double)d, s);
        g += (double)gd;
    }
    __shared__ double red[2][4];
    s = wave_sum_d(s); g = wave_sum_d(g);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = g; }
    __syncthreads();
    if (threadIdx.x == 0) {
        row_sq[b] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        row_g[b] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// loss = (float)((sum_b (double)omega_b * row_sq[b]) / (B HW)), dbias = (float)(sum_b row_g[b]): one thread, rows in
// order, one IEEE fp64 operation per step
__global__ void mse_weighted_finalize_kernel(const double* row_sq, const double* row_g, int B, int HW, const int* t,
                                             const float* w_tab, const float* iw, float* loss_out, float* dbias_out,
                                             int* nonfinite) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0, g = 0.0;
    for (int b = 0; b < B; ++b) {
        const double om = (w_tab || iw) ? (double)tl_omega(t, w_tab, iw, b) : 1.0;
        const double term = om * row_sq[b];
        a = a + term;
        g = g + row_g[b];
    }
    const float loss = (float)(a / ((double)B * (double)HW));
    if (loss_out) *loss_out = loss;
    if (dbias_out) *dbias_out = (float)g;
    if (nonfinite && !isfinite(loss)) *nonfinite += 1;
}

// The record update and (mode 1) the table rebuild: one thread, strictly in the documented order, every fp64 operation
// one IEEE operation (no contraction), so a numpy fp64 restatement reproduces every bit.
__global__ void tloss_record_kernel(const double* row_sq, const int* t, const float* w_tab, int B, int HW, int T, int NB,
                                    double alpha, double* rec, int mode, int warmup, double mix, double* cdf,
                                    float* iw_tab) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double dHW = (double)HW, dT = (double)T;
    for (int b = 0; b < B; ++b) {
        const double l = (row_sq[b] / dHW);
        const int tb = t[b];
        if (!isfinite(l) || tb < 1 || tb > T) continue;
        const int k = (int)(((long long)tb * NB - 1) / T);
        const double wl = w_tab ? ((double)w_tab[tb] * l) : l;
        const double y = (wl * wl);
        double* r = rec + 3 * k;
        const double n = r[0];
        if (n == 0.0) {
            r[1] = l; r[2] = y;
        } else {
            const double m1 = r[1], m2 = r[2];
            r[1] = m1 + alpha * (l - m1);
            r[2] = m2 + alpha * (y - m2);
        }
        r[0] = n + 1.0;
    }
    if (mode != 1) return;
    double nmin = rec[0], Ssum = 0.0;
    for (int k = 0; k < NB; ++k) {
        const double n = rec[3 * k];
        nmin = n < nmin ? n : nmin;
        Ssum = (Ssum + sqrt(rec[3 * k + 2]));
    }
    const bool uniform = nmin < (double)warmup || !isfinite(Ssum) || !(Ssum > 0.0);
    const double omm = (1.0 - mix);
    double run = 0.0;
    for (int k = 0; k < NB; ++k) {
        const int e1 = tl_edge(k + 1, T, NB);
        if (uniform) {
            cdf[k] = ((double)e1 / dT);
            iw_tab[k] = 1.0f;
            continue;
        }
        const double nk = (double)(e1 - tl_edge(k, T, NB));
        const double p1 = (omm * sqrt(rec[3 * k + 2])) / Ssum;
        const double p2 = ((mix * nk) / dT);
        const double q = (p1 + p2);
        run = (run + q);
        cdf[k] = run;
        iw_tab[k] = (float)(nk / (dT * q));
    }
}

// ------------------------------------------ C ABI ------------------------------------------------
CDM_API int cdm_tsample_draw(int* t, float* iw, int B, int T, int NB, const double* cdf, const float* iw_tab,
                             unsigned long long seed, unsigned int sub, const int* sub_dev, void* stream) {
    if (!t || !iw || !cdf || !iw_tab || B < 1 || T < 1 || NB < 1 || NB > T || NB > CDM_TLOSS_MAX_BUCKETS)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tsample_draw_kernel, dim3(nblocks(B)), dim3(256), 0, S(stream), t, iw, B, T, NB, cdf, iw_tab, seed,
                       sub, sub_dev);
    return cdm_status();
}

CDM_API int cdm_mse_weighted(const float* pred, const float* noise, int B, int HW, const int* t, const float* w_tab,
                             const float* iw, double grad_numel, float* dpred, double* row_sq, double* row_g,
                             float* loss_out, float* dbias_out, int* nonfinite, void* stream) {
    if (!pred || !noise || !dpred || !row_sq || !row_g || B < 1 || HW < 1 || !(grad_numel > 0.0) || (w_tab && !t))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mse_weighted_kernel, dim3(B), dim3(256), 0, S(stream), pred, noise, HW, t, w_tab, iw,
                       (float)(2.0 / grad_numel), dpred, row_sq, row_g);
    int e = cdm_status(); if (e) return e;
    hipLaunchKernelGGL(mse_weighted_finalize_kernel, dim3(1), dim3(64), 0, S(stream), row_sq, row_g, B, HW, t, w_tab, iw,
                       loss_out, dbias_out, nonfinite);
    return cdm_status();
}

CDM_API int cdm_tloss_record(const double* row_sq, const int* t, const float* w_tab, int B, int HW, int T, int NB,
                             double alpha, double* rec, int mode, int warmup, double mix, double* cdf, float* iw_tab,
                             void* stream) {
    if (!row_sq || !t || !rec || B < 1 || HW < 1 || T < 1 || NB < 1 || NB > T || NB > CDM_TLOSS_MAX_BUCKETS ||
        !(alpha > 0.0 && alpha <= 1.0) || mode < 0 || mode > 1)
        return (int)hipErrorInvalidValue;
    if (mode == 1 && (!cdf || !iw_tab || warmup < 1 || !(mix > 0.0 && mix <= 1.0))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tloss_record_kernel, dim3(1), dim3(64), 0, S(stream), row_sq, t, w_tab, B, HW, T, NB, alpha, rec,
                       mode, warmup, mix, cdf, iw_tab);
    return cdm_status();
}
