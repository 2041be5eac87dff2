// Observation-guided sampling (diffusion.GuidedDDIMSampler): diffusion posterior sampling against a
// block-averaged, weighted, noisy observation y = A x0 + n.  Two kernels around the engine's frozen forward and full
// backward: the misfit of the data prediction with its gradient at the network output and at the state, and the DDIM
// step followed by the step down the gradient of the misfit norm.  Neither allocates, neither synchronises, the
// position is read from the device.
#include "cdm_common.h"
#include "cdm_hip.h"
#include "sampler_parts.h"

namespace cdm {

// One block per sample; thread t owns the cells t, t + 256, ... of the sample's (H / F)^2 cells, so the F x F mean and
// its adjoint never cross threads.  At the position p = *cur_k, with s = sq[p], r = ra[p], each line one fp32 rounding:
//   x0h_e = (x_e - s eps_e) * r                        eps: cfg_eps
//   m_q   = (x0h of the cell's F*F pixels added in row-major order, the first one the start) * (1 / F^2)
//   r_q   = obs_q - m_q;   wr_q = wgt_q r_q;   u_q = wr_q * (1 / F^2)
//   gdir_e = c_dir u_q,  c_dir = (float)(-2 (double)r);     ge_e = c_eps u_q,  c_eps = (float)(2 (double)s (double)r)
//   deps_e = ge_e without cfg;  w ge_e on the cond row and (1 - w) ge_e on the uncond row with cfg
// and in fp64 L = sum_q ((double)wgt_q (double)r_q) (double)r_q: per-thread sums over the thread's cells ascending, a
// wave64 butterfly, then (w0 + w1) + (w2 + w3) through LDS: the same bits every run.  A cell with wgt_q == 0 is not
// observed: obs_q is not read (it may hold anything), u_q = 0 and L gets nothing from it.
template <int F>
__global__ __launch_bounds__(256) void obs_residual_grad_kernel(const float* x, const float* eps, int cfg, float w,
                                                                const float* obs, const float* wgt, long long wgt_numel,
                                                                int n, int H, const int* cur_k, const float* sq,
                                                                const float* ra, int npos, double* L, double* hist,
                                                                float* deps, float* gdir) {
#pragma clang fp contract(off)  // separate roundings, as the restatement computes them
    const int p = *cur_k;
    if (p < 1 || p > npos) return;                      // block-uniform
    const int smp = blockIdx.x, Hc = H / F, cells = Hc * Hc;
    const long long HW = (long long)H * H, numel = (long long)n * HW, base = (long long)smp * HW;
    const float s = sq[p], r = ra[p];
    const float c_dir = (float)(-2.0 * (double)r), c_eps = (float)((2.0 * (double)s) * (double)r);
    const float wu = 1.f - w;
    constexpr float inv = 1.f / (float)(F * F);
    double acc = 0.0;
    for (int q = threadIdx.x; q < cells; q += 256) {
        const int qr = q / Hc, qc = q - qr * Hc;
        const long long e0 = base + (long long)qr * F * H + (long long)qc * F;
        float sum = 0.f;
#pragma unroll
        for (int a = 0; a < F; ++a)
#pragma unroll
            for (int b = 0; b < F; ++b) {
                const long long e = e0 + (long long)a * H + b;
                const float x0h = (x[e] - s * cfg_eps(eps, numel, e, cfg, w)) * r;
                sum = (a == 0 && b == 0) ? x0h : sum + x0h;
            }
        const float wq = wgt[((long long)smp * cells + q) % wgt_numel];
        float u = 0.f;
        if (wq != 0.f) {
            const float res = obs[(long long)smp * cells + q] - sum * inv;
            const float wr = wq * res;
            acc = acc + ((double)wq * (double)res) * (double)res;
            u = wr * inv;
        }
        if (deps) {
            const float gd = c_dir * u, ge = c_eps * u;
#pragma unroll
            for (int a = 0; a < F; ++a)
#pragma unroll
                for (int b = 0; b < F; ++b) {
                    const long long e = e0 + (long long)a * H + b;
                    gdir[e] = gd;
                    if (cfg) { deps[e] = w * ge; deps[numel + e] = wu * ge; }
                    else deps[e] = ge;
                }
        }
    }
    __shared__ double red[4];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        L[smp] = tot;
        hist[(long long)p * n + smp] = tot;
    }
}

// The position-keyed DDIM step (ddim_step_kernel<true>'s update, key domain and write-out) followed by the guidance
// step: x <- ((cx[k] x + ce[k] eps) + sigma[k] z) - kn grad, grad = (grad_dir + dx) (+ dx of the uncond row with cfg),
// kn = (float)((double)zeta / (2 sqrt(L[sample]))) and no subtraction where L == 0 or zeta == 0 (grad_dir, dx and L
// are then not read: the DDIM step's bits).
__global__ void ddim_step_guided_kernel(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg,
                                        float w, const int* cur_k, const float* cx, const float* ce, const float* sigma,
                                        int S, const float* z_table, long long zstride, unsigned long long seed,
                                        const long long* seed_dev, const int* snap_slot, float* snaps,
                                        const float* grad_dir, const float* dx, const double* L, float zeta,
                                        long long HW) {
#pragma clang fp contract(off)  // separate fp32 roundings, as the restatement computes them
    const int k = *cur_k;
    if (k < 1 || k > S) return;
    const float a = cx[k], c = ce[k], sg = sigma[k];
    const int slot = snap_slot ? snap_slot[k] : -1;
    const unsigned long long sd = run_key(seed, seed_dev) ^ STEP_NOISE_DOMAIN;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (long long)gridDim.x * blockDim.x) {
        float v = ddim_update(xin[e], cfg_eps(eps, numel, e, cfg, w), a, c, sg, z_table, S - k, zstride, sd, (uint32_t)k,
                              e);
        if (zeta != 0.f) {
            const double Ln = L[e / HW];
            if (Ln != 0.0) {
                const float kn = (float)((double)zeta / (2.0 * sqrt(Ln)));
                float g = grad_dir[e] + dx[e];
                if (cfg) g = g + dx[numel + e];
                v = v - kn * g;
            }
        }
        store_state(v, e, numel, x, x2, slot, snaps);
    }
}

}  // namespace cdm

using namespace cdm;
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

CDM_API int cdm_obs_residual_grad(const float* x, const float* eps, int cfg, float w, const float* obs, const float* wgt,
                                  long long wgt_numel, int n, int H, int f, const int* cur_k, const float* sq,
                                  const float* ra, int npos, double* L, double* hist, float* deps, float* gdir,
                                  void* stream) {
    if (!x || !eps || !obs || !wgt || !cur_k || !sq || !ra || !L || !hist || n < 1 || H < 1 || npos < 1 ||
        (f != 1 && f != 2 && f != 4 && f != 8) || H % f != 0 || (deps == nullptr) != (gdir == nullptr))
        return (int)hipErrorInvalidValue;
    const long long cells = (long long)(H / f) * (H / f);
    if (wgt_numel != cells && wgt_numel != cells * n) return (int)hipErrorInvalidValue;
#define CDM_OBS_LAUNCH(F)                                                                                              \
    hipLaunchKernelGGL(obs_residual_grad_kernel<F>, dim3(n), dim3(256), 0, S(stream), x, eps, cfg, w, obs, wgt,        \
                       wgt_numel, n, H, cur_k, sq, ra, npos, L, hist, deps, gdir)
    switch (f) {
        case 1: CDM_OBS_LAUNCH(1); break;
        case 2: CDM_OBS_LAUNCH(2); break;
        case 4: CDM_OBS_LAUNCH(4); break;
        default: CDM_OBS_LAUNCH(8); break;
    }
#undef CDM_OBS_LAUNCH
    return cdm_status();
}

CDM_API int cdm_ddim_step_guided(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg,
                                 float w, const int* cur_k, const float* cx, const float* ce, const float* sigma, int npos,
                                 const float* z_table, long long zstride, unsigned long long seed,
                                 const long long* seed_dev, const int* snap_slot, float* snaps, const float* grad_dir,
                                 const float* dx, const double* L, float zeta, int H, void* stream) {
    if (!xin || !x || !eps || !cur_k || !cx || !ce || !sigma || npos < 1 || numel <= 0 || zstride < 0 ||
        (snap_slot && !snaps) || H < 1 || numel % ((long long)H * H) != 0 || !(zeta >= 0.f) || !(zeta < INFINITY) ||
        (zeta != 0.f && (!grad_dir || !dx || !L)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ddim_step_guided_kernel, dim3(nblocks(numel)), dim3(256), 0, S(stream), xin, x, x2, numel, eps, cfg,
                       w, cur_k, cx, ce, sigma, npos, z_table, zstride, seed, seed_dev, snap_slot, snaps, grad_dir, dx, L,
                       zeta, (long long)H * H);
    return cdm_status();
}
