// conv3x3 weight gradient (kernel-row kernel, split-GEMM fallback): C ABI.  Kernels: conv_kernels.h.
#include "conv_kernels.h"

// the wave order of the kernel-row weight gradient: staggered with every wave loading one K step ahead (default), or
// lock-step ($CDM_WGRAD_STAGGER=0, which the tests hold bit-identical to the default).  Same-box A/Bs of the staggered
// form and of the look-ahead: profiles/r6_ab_wgrad_stagger_early.txt, r6_ab_wgrad_ahead.txt (round 3's form, slower:
// r3_ab_wgrad_stagger.txt); the deeper and the interleaved staging that were measured and dropped:
// r3_ab_deep_staging.txt, r3_ab_wgrad_interleave.txt.
static int wgrad_stagger() {
    static const int v = env_int("CDM_WGRAD_STAGGER", 1) ? WG_STAGGER | WG_AHEAD : 0;
    return v;
}

template <int KS, class PRE = PreNone, class PX = PreNone, class GT = float, class XT = float>
static int launch_wgrad_row(const GT* dy, int lddy, int Cout, const XT* x, int H, int W, int Cin, int ldx, int K,
                            int sp, const float* amax_dy, const float* amax_x, float* slab, int nterm, hipStream_t st,
                            PRE pre = PRE{}, PX px = PX{}) {
    constexpr bool F32 = std::is_same<GT, float>::value && std::is_same<XT, float>::value;
    const int ktiles = K / (16 * KS), per = (ktiles + sp - 1) / sp;
    const dim3 grid((Cout / 128) * 3 * (Cin / 128) * ((ktiles + per - 1) / per));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(512), 0, st, dy, lddy, Cout, x, H, W, Cin, ldx, ktiles, per, amax_dy, amax_x,
                           slab, pre, px, wgrad_stagger());
        return cdm_status();
    };
    if constexpr (!F32) {   // bf16 activations: the one-term (C4) arithmetic only
        if (nterm != 1) return (int)hipErrorInvalidValue;
        return launch(wgrad3x3_row_kernel<1, KS, PRE, PX, GT, XT>);
    } else {
        // 64-pixel K steps (KS 4: one-term 66 KiB of LDS, h3 133 KiB) and the fused X transform: the 16-bit
        // arithmetics (h3, bf16) only
        if (nterm == NT_H3) return launch(wgrad3x3_row_kernel<NT_H3, KS, PRE, PX>);
        if (nterm == 1) return launch(wgrad3x3_row_kernel<1, KS, PRE, PX>);
        if constexpr (KS != 4 && PX::kind == 0) {
            if (nterm == 3) return launch(wgrad3x3_row_kernel<3, KS, PRE, PX>);
            if (nterm == 6) return launch(wgrad3x3_row_kernel<6, KS, PRE, PX>);
        }
        return (int)hipErrorInvalidValue;
    }
}

// conv3x3 weight gradient on the 16-bit matrix cores (same slab contract as cdm_conv3x3_wgrad); W % 8 == 0
static int conv3x3_wgrad_split(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin,
                               int ldx, const float* amax_dy, const float* amax_x, int splits, float* slab, int nterm,
                               hipStream_t st) {
    if (Cin % 4 || Cout % 4 || W % 8) return (int)hipErrorInvalidValue;
    const int M = Cout, NN = 9 * Cin, K = N * H * W;
    const int sp = effective_splits(K, splits);
    EpiStore ep{slab, NN, (long long)M * NN, nullptr, 1, 0, nullptr, 0, M, NN};
    if (Cin % 128 == 0 && Cout % 128 == 0 && lddy % 4 == 0 && ldx % 4 == 0) {   // kernel-row path (3 taps per block)
        if (W % 32 == 0 && effective_splits(K, splits, 32) == sp)               // 32-pixel K steps, else 16
            return launch_wgrad_row<2>(dy, lddy, Cout, x, H, W, Cin, ldx, K, sp, amax_dy, amax_x, slab, nterm, st);
        if (W % 16 == 0 && effective_splits(K, splits, 16) == sp)
            return launch_wgrad_row<1>(dy, lddy, Cout, x, H, W, Cin, ldx, K, sp, amax_dy, amax_x, slab, nterm, st);
    }
    return launch_gemm_x3<ColK<LdDenseAT>::template T, ColK<LdIm2colB>::template T, EpiStore, false>(
        MkColK<LdDenseAT>{LdDenseAT{dy, lddy, M, K}, amax_dy}, MkColK<LdIm2colB>{LdIm2colB{x, H, W, Cin, ldx, K, NN}, amax_x},
        ep, M, NN, K, sp, nterm, st);
}

CDM_API int cdm_conv3x3_wgrad_x3(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin,
                                 int ldx, int splits, float* slab, int nterm, void* stream) {
    if (nterm != 1 && nterm != 3 && nterm != 6) return (int)hipErrorInvalidValue;
    return conv3x3_wgrad_split(dy, lddy, Cout, x, N, H, W, Cin, ldx, nullptr, nullptr, splits, slab, nterm, S(stream));
}

CDM_API int cdm_conv3x3_wgrad_x16(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin,
                                  int ldx, const float* amax_dy, const float* amax_x, int splits, float* slab, int nterm,
                                  void* stream) {
    if (!x16_ok(nterm) || !x16_amax_ok(nterm, amax_dy, amax_x)) return (int)hipErrorInvalidValue;
    return conv3x3_wgrad_split(dy, lddy, Cout, x, N, H, W, Cin, ldx, amax_dy, amax_x, splits, slab, nterm, S(stream));
}

// the kernel-row weight gradient with both staging fusions selectable: g / y / BN coefficients (optional, all or
// none: the dY operand is the BN backward of g, bn_bwd_elem per staged element, dY never written) and x_s / x_t
// (optional: the X operand is relu(x * x_s[c] + x_t[c]) of the previous layer's pre-norm output).  Cin % 128 ==
// Cout % 128 == 0, W % 16 == 0.
CDM_API int cdm_conv3x3_wgrad_x16_ex(const float* g, int ldg, const float* y, int ldy, const float* s, const float* t,
                                     const float* mean, const float* invstd, const float* A, const float* B,
                                     const float* Cc, int Cout, const float* x, int N, int H, int W, int Cin, int ldx,
                                     const float* x_s, const float* x_t, const float* x_g, int ldxg,
                                     const float* x_mean, const float* x_invstd, float* x_sums,
                                     const float* amax_dy, const float* amax_x, int splits, float* slab, int nterm,
                                     int dt, void* stream) {
    if (!x16_ok(nterm) || Cin % 128 || Cout % 128 || W % 16 || ldg % 4 || ldx % 4 ||
        !x16_amax_ok(nterm, amax_dy, amax_x) || (x_s && !x_t) || (y && ldy % 4) ||
        (x_sums && (!x_s || !x_g || ldxg % 4 || !x_mean || !x_invstd)) || (dt && nterm != 1))
        return (int)hipErrorInvalidValue;
    const int K = N * H * W, sp = effective_splits(K, splits);
    const bool ks2 = W % 32 == 0 && effective_splits(K, splits, 32) == sp;
    // 64-pixel K steps for bf16 activations: with fp32 one-term activations they measured 1.81x slower per launch than
    // 32 (1284 vs 710 us, 22 VGPRs spilled, profiles/r3_c4_ks4.txt); the bf16 staging registers are half as wide (249
    // VGPRs, no spill): C4 29.64-29.89 -> 29.31-29.44 ms per step (profiles/r4_ab_dy_store_ks4.txt).  For h3 too, on the
    // 64^2 layers: 133 KiB of LDS (gfx950 has 160 per CU) and 254 VGPRs without spills; same-box A/B, 3 rounds: C2
    // 44.94-45.11 -> 44.66-44.78 ms (profiles/r6_ab_wgrad_ks4h3.txt; 16-pixel steps: 45.70-45.77 -> 47.33-47.38,
    // profiles/r6_ab_wgrad_ks1.txt)
    const bool ks4 = W % 64 == 0 && effective_splits(K, splits, 64) == sp;
    const bool ks4h3 = nterm == NT_H3 && ks4;
    if (!ks2 && effective_splits(K, splits, 16) != sp) return (int)hipErrorInvalidValue;
    const PreBnBwd pre{y, ldy, {s, t, mean, invstd, A, B, Cc}};
    const PreBnRelu px{{x_s, x_t}};
    const PreBnReluSums pxs{{x_s, x_t}, x_g, ldxg, x_mean, x_invstd, x_sums};
    hipStream_t st = S(stream);
    // dt bit 0: g (and y) are bf16, bit 1: x (and x_g) are bf16
    auto run = [&](auto gtag, auto xtag) {
        using GT = decltype(gtag);
        using XT = decltype(xtag);
        const GT* gg = reinterpret_cast<const GT*>(g);
        const XT* xx = reinterpret_cast<const XT*>(x);
        constexpr bool BF = !(std::is_same<GT, float>::value && std::is_same<XT, float>::value);
#define CDM_WG(KS_, PRE_, PX_) launch_wgrad_row<KS_>(gg, ldg, Cout, xx, H, W, Cin, ldx, K, sp, amax_dy, amax_x, slab, \
                                                     nterm, st, PRE_, PX_)
        auto wgk = [&](auto pre_, auto px_) -> int {
            if constexpr (BF) {
                if (ks4) return CDM_WG(4, pre_, px_);
            } else {
                if (ks4h3) return CDM_WG(4, pre_, px_);
            }
            return ks2 ? CDM_WG(2, pre_, px_) : CDM_WG(1, pre_, px_);
        };
#define CDM_WGK(PRE_, PX_) wgk(PRE_, PX_)
        if (x_sums) {   // the producer's BN-backward sums ride along (x_sums[splits][5][Cin])
            if (y) return CDM_WGK(pre, pxs);
            return CDM_WGK(PreNone{}, pxs);
        }
        if (y && x_s) return CDM_WGK(pre, px);
        if (y) return CDM_WGK(pre, PreNone{});
        if (x_s) return CDM_WGK(PreNone{}, px);
        return CDM_WGK(PreNone{}, PreNone{});
#undef CDM_WGK
#undef CDM_WG
    };
    switch (dt & 3) {
        case 1: return run(__bf16{}, float{});
        case 2: return run(float{}, __bf16{});
        case 3: return run(__bf16{}, __bf16{});
        default: return run(float{}, float{});
    }
}
