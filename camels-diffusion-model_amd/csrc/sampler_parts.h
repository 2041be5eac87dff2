// The pieces the kernels that write the sampler state share (csrc/misc.hip: denoise, DDIM, DPM-Solver++, the blends;
// csrc/guide.hip: the observation-guided step; csrc/flow.hip: the flow likelihood): the counter-based noise, the CFG
// combine, the per-run key, the fp64 wave sum and the write-out.  The arithmetic of each update stays in its kernel.
#pragma once
#include "cdm_common.h"

namespace cdm {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (counter-based; used for training noise / timesteps and sampler z)
// ------------------------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };
static __device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}
static __device__ __forceinline__ float u01(uint32_t v) { return ((float)(v >> 8) + 0.5f) * (1.0f / 16777216.0f); }
static __device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = u01(a), u2 = u01(b);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c; sincosf(6.283185307179586f * u2, &s, &c);
    z0 = r * c; z1 = r * s;
}
// normal for element e of stream `sub`
static __device__ __forceinline__ float philox_normal(unsigned long long seed, uint32_t sub, long long e) {
    const U4 v = philox((uint32_t)(e >> 2), (uint32_t)((unsigned long long)e >> 34), sub, 0x5EEDu,
                        (uint32_t)seed, (uint32_t)(seed >> 32));
    float z0, z1, z2, z3;
    box_muller(v.x, v.y, z0, z1); box_muller(v.z, v.w, z2, z3);
    const int j = (int)(e & 3);
    return j == 0 ? z0 : (j == 1 ? z1 : (j == 2 ? z2 : z3));
}

// element e of the stream cdm_philox_uniform(out, n, 0, 1, seed, sub) writes (lo + (hi - lo) u01 is u01 itself there)
static __device__ __forceinline__ float philox_u01_elem(unsigned long long seed, uint32_t sub, long long e) {
    const long long q = e >> 2;
    const U4 r = philox((uint32_t)q, (uint32_t)((unsigned long long)q >> 32), sub, 0x0417u, (uint32_t)seed,
                        (uint32_t)(seed >> 32));
    const int j = (int)(e & 3);
    return u01(j == 0 ? r.x : (j == 1 ? r.y : (j == 2 ? r.z : r.w)));
}

// fp64 sum over the 64 lanes of a wave, every lane gets it: a butterfly (xor 32, 16, ..., 1), the same bits every run
static __device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// eps of a step: eu + w (ec - eu) when cfg (classifier-free guidance; model batch = 2n, cond half first), else eps[e].
static __device__ __forceinline__ float cfg_eps(const float* eps, long long numel, long long e, int cfg, float w) {
#pragma clang fp contract(off)  // per function, so needed here too: a fused w * (ep - eu) + eu is another rounding
    const float ep = eps[e];
    if (!cfg) return ep;
    const float eu = eps[numel + e];
    return eu + w * (ep - eu);
}
// per-run Philox key: seed ^ *seed_dev (drawn from torch's CUDA generator before every run, so consecutive sampling
// calls get fresh z, as the reference's randn_like on the device does)
static __device__ __forceinline__ unsigned long long run_key(unsigned long long seed, const long long* seed_dev) {
    return seed_dev ? seed ^ (unsigned long long)seed_dev[0] : seed;
}
// Writes v into x and both halves of the model-input buffer (x2 may alias x), and a snapshot when slot >= 0.
static __device__ __forceinline__ void store_state(float v, long long e, long long numel, float* x, float* x2, int slot,
                                                   float* snaps) {
    x[e] = v;
    if (x2) { x2[e] = v; x2[numel + e] = v; }
    if (slot >= 0) snaps[(long long)slot * numel + e] = v;
}

// The strided update of a position k: (cx x + ce eps) + sigma z with separate fp32 roundings; z is neither read nor
// drawn where sigma == 0, else row zrow of z_table when given, else Philox(sd, stream sub).
static __device__ __forceinline__ float ddim_update(float xe, float ep, float a, float c, float sg, const float* z_table,
                                                    long long zrow, long long zstride, unsigned long long sd,
                                                    uint32_t sub, long long e) {
#pragma clang fp contract(off)
    float v = a * xe + c * ep;
    if (sg != 0.f) {
        const float z = z_table ? z_table[zrow * zstride + e] : philox_normal(sd, sub, e);
        v = v + sg * z;
    }
    return v;
}

// Key domain of a device z keyed by the position (a position program, where one timestep is visited more than once:
// cdm_ddim_step_pos, cdm_ddim_step_guided).  The constant is the ASCII of "pos_step" and has no other meaning.
constexpr unsigned long long STEP_NOISE_DOMAIN = 0x706F735F73746570ull;
// Key domain of the Rademacher probes of the flow likelihood (csrc/flow.hip), keyed by the position.  The constant is
// the ASCII of "flowprob" and has no other meaning.
constexpr unsigned long long FLOW_PROBE_DOMAIN = 0x666C6F7770726F62ull;

static inline int nblocks(long long total, int per = 256, int cap = 8192) {
    long long b = (total + per - 1) / per;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace cdm
