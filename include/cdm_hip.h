/*
 * cdm_hip.h — C ABI of libcdm_hip.so, the MI355X (gfx950) kernels behind the ContextUnet DDPM
 * hot path.  Plain pointers and sizes only (no torch types).  Every function returns 0 on success
 * or a hipError_t code; launches go on the caller's stream (`stream` is a hipStream_t, NULL =
 * default stream); the library never allocates, never synchronises and keeps no global state, so
 * every call can be captured into a hipGraph.
 *
 * The reference has no FFI: its boundary is the Python module API.  Each entry point
 * below names the reference operation it replaces (paths relative to the reference repo root).
 * Layout: activations NHWC fp32, (N,H,W,C) with a pixel stride `ld*` >= C so that channel slices
 * of concatenation buffers are addressable (replaces torch.cat, diffusion_utilities.py:96 and
 * ContextUnet.py:59).  Weights are the reference OIHW / ConvTranspose [Cin][Cout][kh][kw] tensors
 * repacked by cdm_pack_* into GEMM layouts.
 */
#ifndef CDM_HIP_H
#define CDM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define CDM_EPI_RELU 1
#define CDM_EPI_ACCUM 2

/* returns 2.  Version 1 -> 2: the convolution section lost its forwarding aliases (the `_h3` names that supplied
 * nterm = 4, dt = 0; the `_bnbwd` names that supplied dy_out = NULL or that staged as cdm_conv3x3_wgrad_x16_ex does)
 * and its two `_variant` measurement entries, with the kernels only those launched; DESIGN.md §3.3 lists each removed
 * name with the call that replaces it.  cdm_conv3x3_fwd_h3 alone stays.  No surviving entry point changed. */
int cdm_abi_version(void);
int cdm_device_sync(void);

/* ---- contractions (fp32 MFMA 32x32x2; csrc/gemm_f32.hip) -------------------------------------- */
/* nn.Conv2d(Cin,Cout,3,1,1) forward (diffusion_utilities.py:27,34; ContextUnet.py:36) and, with
 * flipped weights, its input gradient.  y (+)= conv(x) + bias; stats[tile][2][stats_ld] receives
 * per-128-pixel column sums / sums of squares (BatchNorm2d batch statistics, diffusion_utilities.py:28).
 * kc must equal the kc the weights were packed with (cdm_pack_conv3x3). */
int cdm_conv3x3_fwd(const float* x, int N, int H, int W, int Cin, int ldx, const float* wpk, const float* bias,
                    float* y, int ldy, int Cout, int flags, float* stats, int stats_ld, int kc, void* stream);
/* conv3x3 forward, fp32-accurate on the bf16 matrix cores: operands split into nterm-term bf16 sums
 * (nterm 6 = fp32-class, 3 = bf16x3, 1 = bf16); wx3 from cdm_split_bf16x3 of the packed weights.
 * Same semantics as cdm_conv3x3_fwd (nn.Conv2d(.,.,3,1,1) diffusion_utilities.py:27,34). */
int cdm_conv3x3_fwd_x3(const float* x, int N, int H, int W, int Cin, int ldx, const void* wx3, const float* bias,
                       float* y, int ldy, int Cout, int flags, float* stats, int stats_ld, int kc, int nterm,
                       void* stream);
/* conv3x3 weight gradient on the split-bf16 path: same slab contract as cdm_conv3x3_wgrad; W % 8 == 0 */
int cdm_conv3x3_wgrad_x3(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin, int ldx,
                         int splits, float* slab, int nterm, void* stream);
/* fp32 [K][N] (ld ldb) -> [ceil(K/16)][3][N][16] bf16 split terms hi/mid/lo */
int cdm_split_bf16x3(const float* b, long long ldb, int K, int N, void* out, void* stream);
/* ---- 16-bit-arithmetic ("x16") convolutions --------------------------------------------------------------------
 * `nterm` selects the arithmetic: NT_H3 = 4 ("h3", fp32-class on the fp16 matrix cores) or 1 (one bf16 term per operand,
 * fp32 accumulate: BASELINE configuration C4, bf16 mixed precision, with every train-mode Conv -> BatchNorm -> ReLU
 * fusion of the h3 path).
 * h3: each operand is scaled by a power of two derived from its max |.| (device scalars amax_*, see cdm_amax_f32) and
 * split into fp16 hi + lo; 3 cross products (hh, hl, lh) per MAC, fp32 accumulate, exact unscale.  Weight images come
 * from cdm_split_f16x2 of the packed weights with the same amax_w.
 * nterm = 1: the weight images come from cdm_split_bf16x3 (plane 0 is read) and the amax_* operand maxima are ignored
 * (may be null).
 * dt: bf16 activation storage of C4's fused Conv -> BatchNorm -> ReLU chain, one-term (nterm = 1) arithmetic only.
 * Forward / dgrad: bit 0 = the source (x or g, and the BN staging's y) holds bf16, bit 1 = the output is stored as bf16
 * (statistics / maxima of the stored values).  Weight gradient: bit 0 = g / dy (and y) are bf16, bit 1 = x (and x_g) are
 * bf16.  dt = 0: fp32 everywhere (every other arithmetic).
 * Reference ops: nn.Conv2d(.,.,3,1,1) diffusion_utilities.py:27,34 and its autograd; nn.ConvTranspose2d(Cin, Cout, 2, 2)
 * diffusion_utilities.py:86. */
/* conv3x3 forward, same semantics as cdm_conv3x3_fwd; amax_y (optional): running max|y| (atomic) */
int cdm_conv3x3_fwd_x16(const float* x, int N, int H, int W, int Cin, int ldx, const void* wx, const float* amax_x,
                        const float* amax_w, const float* bias, float* y, int ldy, int Cout, int flags, float* stats,
                        int stats_ld, int kc, float* amax_y, int nterm, int dt, void* stream);
/* the plain h3 forward, = cdm_conv3x3_fwd_x16(..., 4, 0): the one retained alias, kept because the benchmark's conv
 * probe calls it */
int cdm_conv3x3_fwd_h3(const float* x, int N, int H, int W, int Cin, int ldx, const void* wx, const float* amax_x,
                       const float* amax_w, const float* bias, float* y, int ldy, int Cout, int flags, float* stats,
                       int stats_ld, int kc, float* amax_y, void* stream);
/* cdm_conv3x3_fwd_x16 with the train-mode Conv -> BatchNorm -> ReLU fusions (LDS-halo shapes only):
 * pre_s / pre_t (optional): the input is relu(x * pre_s[c] + pre_t[c]) computed while staging (x = the previous
 * layer's pre-norm output; its BatchNorm apply is never materialised; *amax_x must be max of that input);
 * ymm (optional, needs stats): per output channel max / min of y as ordered-int keys ymm[c] / ymm[ymm_ld + c],
 * cleared by the caller to INT_MIN / INT_MAX (cdm_fill_i32); cdm_bn_fwd_finalize turns them into max|z| */
int cdm_conv3x3_fwd_x16_ex(const float* x, int N, int H, int W, int Cin, int ldx, const float* pre_s, const float* pre_t,
                           const void* wx, const float* amax_x, const float* amax_w, const float* bias, float* y,
                           int ldy, int Cout, int flags, float* stats, int stats_ld, int kc, float* amax_y, int* ymm,
                           int ymm_ld, int nterm, int dt, void* stream);
/* eval-mode conv3x3 of a Conv -> BatchNorm (folded into wx / bias) -> ReLU layer with its output transform in the
 * LDS-halo epilogue (csrc/conv_fwd_eval.hip; W == H in {32, 64}, kc = 16, Cout % 128 == 0), v = relu(conv + bias):
 *   kind 1 (resid, diffusion_utilities.py:54-55): y[p][c] = sc_w[s][c] sc_x[p] + sc_b[s][c] + v, s = image >= split
 *   kind 2 (FiLM, ContextUnet.py:57-58):           y[p][c] = fa[image * fan + c] v + fb[image * fbn + c]
 *   kind 3 (MaxPool2d(2), diffusion_utilities.py:109): y = the [N][H/2][W/2] pooled map (row stride ldy)
 * amax_y (h3): running max|y|.  Replaces cdm_conv3x3_fwd_x16 + cdm_norm_apply_fwd of the eval forward. */
int cdm_conv3x3_fwd_x16_fused(const float* x, int N, int H, int W, int Cin, int ldx, const void* wx,
                              const float* amax_x, const float* amax_w, const float* bias, float* y, int ldy, int Cout,
                              int kc, float* amax_y, int kind, const float* sc_x, const float* sc_w, const float* sc_b,
                              int split, const float* fa, int fan, const float* fb, int fbn, int nterm, void* stream);
/* tiles-per-block hook of the shipped h3 LDS-halo conv (64x64 maps, no bias / stats; tests): the low 16 bits of abl
 * must be 1 (the retired timing-ablation masks return hipErrorInvalidValue and launch nothing); bits 16+: tiles per
 * block (0 -> 1) in place of the launcher's own policy */
int cdm_conv3x3_halo_ablate(int abl, const float* x, int N, int H, int Cin, int ldx, const void* wx,
                            const float* amax_x, const float* amax_w, float* y, int ldy, int Cout, void* stream);
/* conv3x3 weight gradient, same slab contract as cdm_conv3x3_wgrad; W % 8 == 0.  Cin % 128 == Cout % 128 == 0 and
 * W % 16 == 0: the kernel-row kernel (3 taps per block; 32-pixel K steps when W % 32 == 0, else 16), other shapes the
 * generic split GEMM */
int cdm_conv3x3_wgrad_x16(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin, int ldx,
                          const float* amax_dy, const float* amax_x, int splits, float* slab, int nterm, void* stream);
/* Conv -> BatchNorm -> ReLU backward, the data gradient, with the BN backward fused into the conv staging:
 * dy = A (y s + t > 0 ? g : 0) + B + Cc (y - mean) invstd per element (the expression of cdm_norm_apply_bwd mode 0,
 * bit-identical), s/t/mean/invstd/A/B/Cc per channel.  LDS-halo kernel, W == H in {32, 64, 128}, C % 16 == 0, C <= 256,
 * C = BN channels, Cout = dgrad output channels, wx = split packed dgrad weights; max|dy| <= *amax_dy from
 * cdm_bn_bwd_amax_bound.
 * dy_out (optional): the dy computed in the staging is also stored there ([pix][C], g's row stride ldg and element
 * type) for the layer's weight gradient (cdm_conv3x3_wgrad_x16_ex with g = dy_out, y = null): the BN backward is
 * evaluated once per element instead of again in each of the weight gradient's 3 kernel-row blocks.  dy_out null: dy is
 * never written. */
int cdm_conv3x3_dgrad_x16_bnbwd_dy(const float* g, int ldg, const float* y, int ldy, const float* s, const float* t,
                                   const float* mean, const float* invstd, const float* A, const float* B,
                                   const float* Cc, int N, int H, int W, int C, const void* wx, const float* amax_dy,
                                   const float* amax_w, float* out, int ldo, int Cout, int flags, float* amax_out,
                                   void* dy_out, int nterm, int dt, void* stream);
/* the kernel-row weight gradient with its staging fusions selectable (Cin % 128 == Cout % 128 == 0, W % 16 == 0; same
 * slab contract as cdm_conv3x3_wgrad; K steps of 64, 32 or 16 pixels by W and the arithmetic):
 * y (+ s, t, mean, invstd, A, B, Cc) non-null: dY = the BatchNorm backward of g, the expression of
 * cdm_conv3x3_dgrad_x16_bnbwd_dy with max|dY| <= *amax_dy from cdm_bn_bwd_amax_bound (dY never written), else dY = g;
 * x_s / x_t non-null: the X operand is relu(x * x_s[c] + x_t[c]) of the previous layer's pre-norm output x.
 * (x_g, ldxg, x_mean, x_invstd, x_sums), all optional (x_sums null: off): with x_s / x_t given, the BatchNorm-backward
 * channel sums of the layer that produced x are accumulated while x is staged:
 * g_pre = (x x_s + x_t > 0 ? x_g : 0), xhat = (x - x_mean) x_invstd; x_sums[(split * 3 + kernel row) * (Cout / 128) +
 * co tile][5][Cin] (one partial per block, splits = effective split count) rows 0 = sum g_pre, 1 = sum g_pre xhat,
 * 4 = sum xhat (rows 2, 3 zero) — the slab of cdm_norm_bwd_reduce mode 0 with 3 Cout/128 tiles per split
 * (x_g = the gradient wrt this conv's input, written by this layer's dgrad before this call). */
int cdm_conv3x3_wgrad_x16_ex(const float* g, int ldg, const float* y, int ldy, const float* s, const float* t,
                             const float* mean, const float* invstd, const float* A, const float* B, const float* Cc,
                             int Cout, const float* x, int N, int H, int W, int Cin, int ldx, const float* x_s,
                             const float* x_t, const float* x_g, int ldxg, const float* x_mean, const float* x_invstd,
                             float* x_sums, const float* amax_dy, const float* amax_x, int splits, float* slab,
                             int nterm, int dt, void* stream);
/* nn.ConvTranspose2d(Cin, Cout, 2, 2) forward and backward (same semantics as cdm_convT2x2_fwd / _dgrad / _wgrad
 * below; H, W = input grid).  fwd: wx = the split image of wpk [Cin][4*Cout] with max|wpk| = *amax_w; dgrad: wx = the
 * split image of wpkT [4 Cout][Cin] (max|W| = *amax_w), max|dy| = *amax_dy; wgrad: max|x| = *amax_x, max|dy| =
 * *amax_dy, W % 8 == 0. */
int cdm_convT2x2_fwd_x16(const float* x, int N, int H, int W, int Cin, int ldx, const void* wx, const float* amax_x,
                         const float* amax_w, const float* bias, float* y, int ldy, int Cout, float* amax_y, int nterm,
                         void* stream);
int cdm_convT2x2_dgrad_x16(const float* dy, int N, int H, int W, int Cout, int lddy, const void* wx,
                           const float* amax_dy, const float* amax_w, float* dx, int lddx, int Cin, int flags, int nterm,
                           void* stream);
int cdm_convT2x2_wgrad_x16(const float* x, int N, int H, int W, int Cin, int ldx, const float* dy, int Cout, int lddy,
                           const float* amax_x, const float* amax_dy, int splits, float* slab, int nterm, void* stream);
/* fp32 [K][N] (ld ldb) -> [ceil(K/16)][3][N][16]: planes 0/1 = fp16 hi/lo of b * 2^(14-e), max|b| = *amax < 2^e */
int cdm_split_f16x2(const float* b, long long ldb, int K, int N, const float* amax, void* out, void* stream);
/* batched train-mode repack: jobs_dev = device array of njobs records
 *   { const float* W (OIHW); int Cin, Cout, kc, pad; bf16* wpk_x; bf16* wdg_x (may be null); float* amax; }
 * (64-bit pointers, 48 bytes per record); writes max|W| (atomic max into a cleared *amax) and the two h3 split
 * images of cdm_pack_conv3x3 + cdm_split_f16x2 directly from W.  max_w_elems = the largest Cout * Cin * 9. */
int cdm_pack_split_conv3x3_batch(const void* jobs_dev, int njobs, long long max_w_elems, void* stream);
/* *out = max(accumulate ? *out : 0, max |x[r*ld + c]|), r < rows, c < C (atomic max, graph-capturable) */
int cdm_amax_f32(const float* x, long long rows, int C, long long ld, float* out, int accumulate, void* stream);
/* ---- sample statistics (csrc/stats.hip) --------------------------------------------------------
 * power[b][u][v] = |sum_{x,y} img[b][x][y] e^{-2 pi i (u x + v y) / N}|^2 * scale, fp64 (direct DFT; T = scratch of
 * B*N*N complex doubles).  scale 1/N^2 = np.fft.fftn(norm="ortho") of power_spectrum, diffusion_utilities.py:322;
 * scale 1 = np.fft.fft2 of calculate_power_spectrum_2d, sample_power_spectra.py:128. */
int cdm_dft2_power(const float* img, int B, int N, double scale, void* T, double* power, void* stream);
/* power[b] = |fftn(box[b])|^2 * scale, fp64, for B row-major boxes of rank 1..3 with extents dims[0..rank) (host
 * array): one direct-DFT pass per axis; T0, T1 = scratch of B * prod(dims) complex doubles each.  The 3-D and non-square
 * branches of power_spectrum (diffusion_utilities.py:316-336). */
int cdm_dftn_power(const float* box, int B, int rank, const int* dims, double scale, void* T0, void* T1, double* power,
                   void* stream);
/* cdm_dftn_power for fp64 boxes: power_spectrum of a float64 numpy box, whose np.fft.fftn runs on the fp64 values
 * (diffusion_utilities.py:322) — no fp32 rounding of the input. */
int cdm_dftn_power_f64(const double* box, int B, int rank, const int* dims, double scale, void* T0, void* T1,
                       double* power, void* stream);
/* out[b][k] = sum_{i = off[k]}^{off[k+1]-1} power[b][idx[i]] in list order (the reference's binning loops,
 * diffusion_utilities.py:352-356 / sample_power_spectra.py:157-163, with the bin geometry built on the host) */
int cdm_bin_sum(const double* power, int B, long long NN, const int* off, const int* idx, int nbins, double* out,
                void* stream);
/* out[b] = np.histogram(x[b], edges[0..nbins], density=True)[0]  (train_diffusion.py:205-207) */
int cdm_histogram_density(const float* x, int B, long long P, const double* edges, int nbins, double* out,
                          void* stream);
/* ---- CAMELS map preprocessing (csrc/data.hip; code/train_diffusion_condition.py:137-144) ----------------------- */
/* out[0], out[1] = min, max of x[0..n) (keys = 2 unsigned of scratch; order-independent atomics) */
int cdm_minmax_f32(const float* x, long long n, unsigned* keys, float* out, void* stream);
/* dst[N][O][O] = bilinear(O x O, align_corners=False)((log10(shift(src) / max) - min) / (max - min)) of src[N][S][S],
 * with minmax = cdm_minmax_f32 of the whole raw dataset (every step of the reference is monotone) */
int cdm_camels_maps(const float* src, int N, int S, int O, const float* minmax, float* dst, void* stream);
/* p[0..n) = 0 (a fill kernel: graph-capturable; a captured hipMemsetAsync did not clear reliably on replay) */
int cdm_zero_f32(float* p, long long n, void* stream);
/* Producers below (cdm_norm_apply_fwd / _bwd, cdm_convT2x2_fwd, cdm_conv3x3_fwd_h3 amax_y) take an optional
 * float* amax: when non-null they atomically max the |values| they store into it, so the next h3 conv gets
 * its operand's max without a separate pass. */
/* nn.ConvTranspose2d(Cin,Cout,2,2) forward (diffusion_utilities.py:86); H,W = input grid. */
int cdm_convT2x2_fwd(const float* x, int N, int H, int W, int Cin, int ldx, const float* wpk, const float* bias,
                     float* y, int ldy, int Cout, float* amax, void* stream);
/* its input gradient (autograd of diffusion_utilities.py:86). */
int cdm_convT2x2_dgrad(const float* dy, int N, int H, int W, int Cout, int lddy, const float* wpkT, float* dx,
                       int lddx, int Cin, int flags, void* stream);
/* dense C = A.B (+bias[n % bias_mod]): up0 ConvTranspose2d(2nf,2nf,h/4,h/4) on a 1x1 map (ContextUnet.py:27)
 * and its input gradient (split-K partial slabs when splits > 1). */
int cdm_gemm_f32(const float* a, long long lda, int M, int K, const float* b, long long ldb, int N, float* c,
                 long long ldc, const float* bias, int bias_mod, int flags, int splits, float* slab, void* stream);
int cdm_gemm_splits(int K, int splits);
/* C[m][n] = A[m][k] . B[k][n] + bias[n % bias_mod] on the 16-bit matrix cores (nterm 4 = h3, 1 = bf16); wx = the split
 * image of B [K][N] (cdm_split_f16x2 with max|B| in *amax_w / cdm_split_bf16x3); h3: max|A| = *amax_a; amax_c
 * (optional): running max|C|.  The up0 ConvTranspose2d(k = h/4) of the 1x1 map (ContextUnet.py:26-30). */
int cdm_gemm_x16(const float* a, long long lda, int M, int K, const void* wx, const float* amax_a, const float* amax_w,
                 int N, float* c, long long ldc, const float* bias, int bias_mod, float* amax_c, int nterm,
                 void* stream);
/* weight gradients (autograd of the layers above), split-K partial slabs [splits][M][N]. */
int cdm_conv3x3_wgrad(const float* dy, int lddy, int Cout, const float* x, int N, int H, int W, int Cin, int ldx,
                      int splits, float* slab, void* stream);
int cdm_convT2x2_wgrad(const float* x, int N, int H, int W, int Cin, int ldx, const float* dy, int Cout, int lddy,
                       int splits, float* slab, void* stream);
int cdm_gemm_tn_f32(const float* a, long long lda, int M, int K, const float* b, long long ldb, int N, int splits,
                    float* slab, void* stream);
/* out[m*s_m + (n/csplit)*s_hi + (n%csplit)*s_lo] (+)= scale * sum_z slab[z][m][n] */
int cdm_slab_reduce(const float* slab, int splits, int M, int N, float* out, long long s_m, long long s_hi,
                    long long s_lo, int csplit, int accumulate, float scale, void* stream);

/* ---- normalisation / pooling / FiLM (csrc/norm.hip) ------------------------------------------- */
/* per-(image, pixel-chunk) partial sums (slab[N][chunks][R][C]).  The chunked reducers (cdm_reduce_stats, _stats_mm,
 * _sum, cdm_norm_bwd_reduce) take 4 <= C <= 1024, C % 4 == 0; any other C returns hipErrorInvalidValue before a
 * launch (C = 0 would divide by zero in the lane split 256 / (C / 4)) and writes nothing. */
int cdm_reduce_stats(const float* y, int ldy, int N, int HW, int C, int csize, float* slab, void* stream);
/* cdm_reduce_stats (identical slab) + optional (ymm != NULL) per-channel max / min of y as ordered-int keys, atomic max
 * into ymm[c] / min into ymm[ymm_ld + c] (cleared by the caller to INT_MIN / INT_MAX): the C_in = 1 init conv's
 * BatchNorm statistics when its BN-ReLU apply runs in the next conv's staging. */
int cdm_reduce_stats_mm(const float* y, int ldy, int N, int HW, int C, int csize, float* slab, int* ymm, int ymm_ld,
                        void* stream);
int cdm_reduce_sum(const float* g, int ldg, int N, int HW, int C, int csize, float* slab, void* stream);
/* BatchNorm2d / GroupNorm(8) + ReLU (+MaxPool2d(2) | +FiLM) backward sums (mode 0 plain, 1 pool, 2 FiLM) */
int cdm_norm_bwd_reduce(int mode, const float* g, int ldg, const float* y, int ldy, int N, int H, int W, int C,
                        const float* s, const float* t, int sn, const float* mean, const float* invstd, int mn,
                        int cpg, const float* film_a, int film_an, int csize, float* slab, void* stream);
/* stage 1 of every slab fold: part[s][r][c] = sum_{tiles of split s} slab[t][r][c] in fp64 (parallel) */
int cdm_slab_colsum(const float* slab, int ntiles, int R, int C, double* part, int splits, void* stream);
/* BatchNorm2d train statistics + running-stat update (diffusion_utilities.py:28,35; momentum 0.1, eps 1e-5).  momentum
 * is a double (torch's own scalar type): the update is formed in fp64 and rounded once. */
int cdm_bn_fwd_finalize(const double* part, int nparts, int R, int C, double count, const float* gamma,
                        const float* beta, float* rmean, float* rvar, long long* nbt, double momentum, float eps,
                        float* mean, float* invstd, float* scale, float* shift, const int* ymm, int ymm_ld,
                        float* amax_z, void* stream);
/* (ymm optional: the per-channel max / min keys of the layer's y from cdm_conv3x3_fwd_x16_ex; amax_z then receives
 *  the exact max over the layer of relu(fmaf(y, scale, shift)) by an atomic max, for the consumer's h3 scale) */
/* p[0..n) = v */
int cdm_fill_i32(int* p, long long n, int v, void* stream);
/* BatchNorm2d eval (running statistics) */
int cdm_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                       float* mean, float* invstd, float* scale, float* shift, void* stream);
/* GroupNorm(8, C) statistics (ContextUnet.py:28,37) */
int cdm_gn_fwd_finalize(const float* slab, int N, int nchunks, int R, int C, int G, double count, const float* gamma,
                        const float* beta, float eps, float* mean, float* invstd, float* scale, float* shift,
                        void* stream);
int cdm_bn_bwd_finalize(const double* part, int nparts, int C, double count, const float* gamma, const float* invstd,
                        float* dgamma, float* dbeta, float* A, float* B, float* Cc, float* dbias, void* stream);
/* eval-mode BatchNorm in the train-structured forward / backward (gradients through model.eval(), the reference's
 * batch_norm(training=False) under autograd): coefficients from the running statistics (running stats and
 * num_batches_tracked untouched; ymm / amax_z as cdm_bn_fwd_finalize), and the backward finalize with the batch terms
 * dropped (A = gamma invstd, B = Cc = 0, dgamma = S2, dbeta = S1, dbias = A S1) */
int cdm_bn_fwd_frozen(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                      float* mean, float* invstd, float* scale, float* shift, const int* ymm, int ymm_ld, float* amax_z,
                      void* stream);
int cdm_bn_bwd_finalize_frozen(const double* part, int nparts, int C, double count, const float* gamma,
                               const float* invstd, float* dgamma, float* dbeta, float* A, float* B, float* Cc,
                               float* dbias, void* stream);
int cdm_gn_bwd_finalize(const float* slab, int N, int nchunks, int C, int G, double count_g, int HW,
                        const float* gamma, const float* invstd, float* A, float* B, float* Cc, float* pdg, float* pdb,
                        float* pdbias, void* stream);
int cdm_slab_sum_nc(const float* slab, int N, int nchunks, int R, int r, int C, float* out, void* stream);
int cdm_col_sum(const float* in, int N, int C, float* out, int accumulate, void* stream);
/* up to three column sums out_k[c] = sum_n in_k[n][c] in one launch.  in1 / in2 may be null, as a suffix: one pair
 * (in1 = in2 = NULL), two (in2 = NULL) or three.  in2 without in1, or any given input without its output, returns
 * hipErrorInvalidValue before a launch. */
int cdm_col_sum3(const float* in0, float* out0, const float* in1, float* out1, const float* in2, float* out2, int N,
                 int C, void* stream);
/* out = [MaxPool2d(2)]([cemb*](ReLU(y*s+t))[+temb])[+ 1x1 shortcut(x)]  — flags 1 pool, 2 FiLM, 4 resid, 8 relu
 * (BN/GN apply diffusion_utilities.py:28-29; MaxPool2d :109; random shortcut :54-55; FiLM ContextUnet.py:57-58) */
int cdm_norm_apply_fwd(int flags, const float* y, int ldy, int N, int H, int W, int C, const float* s, const float* t,
                       int sn, const float* film_a, int film_an, const float* film_b, int film_bn, const float* rx,
                       const float* rw, const float* rb, int rsplit, float* out, int ldo, float* amax, void* stream);
/* the same residual apply for in_channels = xc > 1 (ContextUnet.py:6,14 — init_conv = ResidualConvBlock(in_channels,
 * n_feat, is_res=True), the 1x1 shortcut of diffusion_utilities.py:54-55 over xc channels):
 * out = [relu](y*s+t) + rb[c] + sum_k rw[c][k] rx[p*ldx + k]; rw [2][C][xc] / rb [2][C] when rsplit < N */
int cdm_norm_apply_fwd_resid_c(int relu, const float* y, int ldy, int N, int H, int W, int C, const float* s,
                               const float* t, const float* rx, int ldx, int xc, const float* rw, const float* rb,
                               int rsplit, float* out, int ldo, float* amax, void* stream);
int cdm_norm_apply_bwd(int mode, const float* g, int ldg, const float* y, int ldy, int N, int H, int W, int C,
                       const float* s, const float* t, int sn, const float* mean, const float* invstd, int mn, int cpg,
                       const float* film_a, int film_an, const float* A, const float* B, const float* Cc, int cn,
                       float* dy, int lddy, float* amax, void* stream);
/* *amax_dy = max(*amax_dy, max_c |A| max|g| + |B| + |Cc| (max|y| + |mean|) invstd): an upper bound of max|dy| of
 * the fused BN backward (from the producers' max|g| = *amax_g and max|y| = *amax_y); one block */
/* dense BatchNorm backward of a bf16-activation (C4) layer as its own pass: dy[p][c] = the fused staging's
 * bn_bwd_elem(g, y) (s, t, mean, invstd, A, B, Cc per channel), P pixels x C channels (C % 8 == 0); dt bit 0: g and y
 * are bf16, bit 1: dy is stored as bf16 (round to nearest even) */
int cdm_bn_bwd_dy(const void* g, int ldg, const void* y, int ldy, long long P, int C, const float* s, const float* t,
                  const float* mean, const float* invstd, const float* A, const float* B, const float* Cc, void* dy,
                  int lddy, int dt, void* stream);
int cdm_bn_bwd_amax_bound(int C, const float* A, const float* B, const float* Cc, const float* mean,
                          const float* invstd, const float* amax_g, const float* amax_y, float* amax_dy, void* stream);

/* ---- small ops (csrc/misc.hip) ---------------------------------------------------------------- */
/* init_conv.conv1: Conv2d(1, nf, 3, 1, 1) (ContextUnet.py:14 -> diffusion_utilities.py:27) */
int cdm_conv3x3_cin1_fwd(const float* x, int N, int H, int W, const float* wt, const float* bias, float* y, int ldy,
                         int C, int relu, float* amax, void* stream);   /* amax: optional running max|y| (atomic) */
int cdm_conv3x3_cin1_wgrad(const float* dy, int lddy, const float* x, int N, int H, int W, int C, int csize,
                           float* slab, void* stream);
/* cdm_conv3x3_cin1_wgrad of the init conv's Conv -> BatchNorm -> ReLU with its BN backward applied while reading: g =
 * grad of the ReLU output, y = pre-norm activations, per-channel s, t, mean, invstd, A, B, Cc as cdm_norm_apply_bwd
 * mode 0 (bit-identical dy, never written).  Replaces the autograd BatchNorm2d backward + Conv2d weight grad of
 * ContextUnet.py:14 (init_conv.conv1, diffusion_utilities.py:26-30). */
int cdm_conv3x3_cin1_wgrad_bnbwd(const float* g, int ldg, const float* y, int ldy, const float* s, const float* t,
                                 const float* mean, const float* invstd, const float* A, const float* B, const float* Cc,
                                 const float* x, int N, int H, int W, int C, int csize, float* slab, void* stream);
int cdm_slab_sum_all(const double* part, int nparts, int R, int r0, int rn, int C, float* out, long long s_r,
                     long long s_c, int accumulate, void* stream);
/* out.3: Conv2d(nf, 1, 3, 1, 1) (ContextUnet.py:39) */
int cdm_conv3x3_cout1_fwd(const float* z, int ldz, int N, int H, int W, int C, const float* w, const float* bias,
                          float* out, void* stream);
/* out.3 on out.1's pre-norm output y with its GroupNorm + ReLU applied while staging (gs / gt per (sample, channel),
 * [N][C]; bit-identical to cdm_norm_apply_fwd then cdm_conv3x3_cout1_fwd): eval forwards (ContextUnet.py:37-39).
 * C % 16 == 0, W | 256, (256 / W) | H. */
int cdm_conv3x3_cout1_fwd_gn(const float* y, int ldy, int N, int H, int W, int C, const float* gs, const float* gt,
                             const float* w, const float* bias, float* out, void* stream);
/* image gradient of the init conv (ResidualConvBlock(1, nf, is_res) under autograd, diffusion_utilities.py:45-55):
 * dx[n][p] = sum_{tap,c} w9[c][8 - tap] dy1[p + tap][c] + sum_c scw[(n >= split) * C + c] gres[p][c], w9 = conv1's OIHW
 * weights [C][1][3][3]; dy1 = the BatchNorm + ReLU backward of g1 with y1 and the coefficients of cdm_norm_apply_bwd
 * mode 0 (y1 == NULL: g1 is dy1); gres = the gradient of the block output (NULL: no shortcut term). */
int cdm_conv3x3_cin1_dgrad(const float* g1, int ldg, const float* y1, int ldy, const float* s, const float* t,
                           const float* mean, const float* invstd, const float* A, const float* B, const float* Cc,
                           const float* w9, const float* gres, int ldr, const float* scw, int split, int N, int H,
                           int W, int C, float* dx, void* stream);
int cdm_conv3x3_cout1_dgrad(const float* deps, int N, int H, int W, int C, const float* w, float* dz, int lddz,
                            void* stream);
/* weight gradient partials: csize > 0: per (image, csize-pixel chunk) [N][chunks][9][C]; csize = -R (band form, H % R
 * == 0): one block per R whole rows, every z pixel read once, partials [N * H / R][9][C] */
int cdm_conv3x3_cout1_wgrad(const float* deps, const float* z, int ldz, int N, int H, int W, int C, int csize,
                            float* slab, void* stream);
/* band form (csize = -R) on out.1's pre-norm output y with its GroupNorm + ReLU (per (n, c) gs / gt, [N][C]) applied
 * while staging: z = relu(y gs + gt), bit-identical to the applied tensor, never materialised */
int cdm_conv3x3_cout1_wgrad_gn(const float* deps, const float* y, int ldy, int N, int H, int W, int C, const float* gs,
                               const float* gt, int csize, float* slab, void* stream);
/* to_vec: AvgPool2d(h/4) + GELU (ContextUnet.py:17) */
int cdm_avgpool_gelu_fin(const float* sums, int N, int C, int HW, float* hpre, float* hv, void* stream);
int cdm_avgpool_gelu_bwd(const float* dhv, const float* hpre, int N, int HW, int C, float* dst, int ldd, void* stream);
/* EmbedFC x4 (diffusion_utilities.py:118-145); `P` points to a host struct cdm_mlp4 (see csrc/misc.hip MlpDesc) */
int cdm_embed_fwd(const void* P, void* stream);
/* input gradient of the two EmbedFCs fed one input (t: timeembed1/2, c: contextembed1/2; ContextUnet.py:51-54):
 * dx[b][k] = sum_i dpre_a[b][i] w1_a[i][k] + sum_i dpre_b[b][i] w1_b[i][k]  (dpre from cdm_embed_bwd, w1 [E][in_dim]) */
int cdm_embed_input_grad(const float* dpre_a, const float* w1_a, int Ea, const float* dpre_b, const float* w1_b, int Eb,
                         int rows, int in_dim, float* dx, void* stream);
int cdm_embed_bwd(const void* P, void* stream);
/* perturb_input (code/train_diffusion_condition.py:202-203) + t/T for the time embedding (:225).
 * t: per-sample steps, or cur_i: one device-side step for the batch with noise row (T - *cur_i)*nstride. */
int cdm_perturb(const float* x, const float* noise, const int* t, const int* cur_i, long long nstride,
                const float* sab, const float* omab, int N, int HW, int T, float* out, float* tin, void* stream);
/* per-sample weighted MSE accumulation of the likelihood / ELBO estimators
 * (code/train_diffusion_elbo.py:74-149; code/train_diffusion_paper.py:77-183):
 * acc[n] += (mean (pred - noise)^2 * mul[i]) / div[i], i = t[n] or *cur_i (noise row (T - i)*nstride) */
int cdm_mse_accum(const float* pred, const float* noise, long long nstride, int T, int N, int HW, const int* t,
                  const int* cur_i, const float* mul, const float* div, float* acc, void* stream);
/* Parameter scan (likelihood.ParamScan, not in the reference): M maps scored under K candidate contexts each, on the
 * same perturbed input; the model batch is M K rows, row m K + k = (map m, candidate k).  One step is cdm_scan_prologue,
 * the noise (cdm_philox_normal with sub_dev = cur_p, or cdm_scan_noise_row), cdm_scan_perturb, the eval forward and
 * cdm_scan_mse_accum; none of them synchronises, and the step index is read from the device.
 * cdm_scan_prologue: the step prologue over a position table.  The counter holds the position p = 0..npos-1 and counts
 * up; pos_t[p] is the timestep of position p, any value of 1..T at any position, so a timestep may repeat and npos may
 * exceed T (cdm_sample_prologue_sub walks a strictly increasing subsequence with npos <= T and counts down).
 *   p = *ctr; *ctr = p + 1; *cur_p = p; *cur_i = i = pos_t[p]; *t_cur = (float)((double)i / T); sc_cur = row p of
 *   sc_table (sc_row floats; sc_table optional).
 * A counter outside 0..npos-1, or a pos_t[p] outside 1..T, sets *cur_i = 0 and writes nothing else; the scan kernels of
 * that step then write nothing.  hipErrorInvalidValue, nothing launched: a required pointer null, npos < 1, T < 1,
 * sc_table without sc_cur. */
int cdm_scan_prologue(int* ctr, int npos, int T, const int* pos_t, int* cur_i, int* cur_p, float* t_cur,
                      const float* sc_table, int sc_row, float* sc_cur, void* stream);
/* out[0..n) = table[*cur_p * n ..]: the noise of the current position out of a pre-drawn table [npos][n].  A *cur_p
 * outside 0..npos-1 writes nothing.  hipErrorInvalidValue: a pointer null, npos < 1, n < 1. */
int cdm_scan_noise_row(const float* table, const int* cur_p, int npos, long long n, float* out, void* stream);
/* out[(m K + k) HW + e] = sab[i] x0[m HW + e] + omab[i] noise[m HW + e] for every k < K, i = *cur_i: x0, noise [M][HW],
 * out [M K][HW].  The expression and fp32 roundings of cdm_perturb: out is bit-identical to cdm_perturb (cur_i form,
 * nstride 0) on x0 and noise with every row repeated K times.  Each source element is read once and stored to the K
 * rows it feeds.  An i outside 1..T writes nothing.  hipErrorInvalidValue, nothing launched: a pointer null; M, K, HW
 * or T < 1. */
int cdm_scan_perturb(const float* x0, const float* noise, const int* cur_i, const float* sab, const float* omab, int M,
                     int K, int HW, int T, float* out, void* stream);
/* acc[m ld + k0 + k] += ((double)w[i] * sum_e (double)d (double)d) / HW with d = pred[(m K + k) HW + e] - noise[m HW + e]
 * formed in fp32, i = *cur_i; pred [M K][HW], noise [M][HW], w [T + 1] fp32, acc fp64 [M][ld] (this call owns columns
 * k0 .. k0 + K - 1).  One block per row; per-thread fp64 sums over a fixed element set, a wave64 butterfly, then a
 * fixed-order fold of the four wave sums through LDS: two runs give the same bits; no atomics.  An i outside 1..T
 * writes nothing.  hipErrorInvalidValue, nothing launched: a pointer null; M, K, HW or T < 1; k0 < 0; ld < k0 + K. */
int cdm_scan_mse_accum(const float* pred, const float* noise, int M, int K, int HW, const int* cur_i, const float* w,
                       int T, double* acc, int ld, int k0, void* stream);
/* Parameter fit (likelihood.ParamFit, not in the reference; csrc/fit.hip): gradient descent on the scan score over the
 * conditioning vector.  A step is cdm_scan_prologue, the noise, cdm_scan_perturb, the frozen train-structured forward,
 * cdm_fit_mse_grad, the engine backward up to the embeddings (dc) and cdm_fit_grad_accum; cdm_fit_update closes a pass
 * over all positions.  None of them synchronises or allocates.
 * cdm_fit_mse_grad: cdm_scan_mse_accum's term with the 1 / R folded in, and the objective's gradient at the network
 * output in the same pass:
 *   d = pred[(m K + k) HW + e] - noise[m HW + e]                         fp32
 *   acc[m ld + k0 + k] += (((double)w[i] * sum_e (double)d (double)d) / HW) * inv_R
 *   deps[(m K + k) HW + e] = coef * d,  coef = (float)(((2.0 * (double)w[i]) * inv_R) / HW)    one fp32 product
 * i = *cur_i; an i outside 1..T writes nothing (acc and deps keep their bits).  Any HW >= 1: float4 loads / stores on
 * the 16-byte aligned body of a row, scalar head and tail.  One block per row, per-thread fp64 sums over a fixed
 * element set, a wave64 butterfly, a fixed-order fold: two runs give the same bits; no atomics.
 * hipErrorInvalidValue, nothing launched: a pointer null; M, K, HW or T < 1; k0 < 0; ld < k0 + K; inv_R <= 0. */
int cdm_fit_mse_grad(const float* pred, const float* noise, int M, int K, int HW, const int* cur_i, const float* w,
                     int T, double inv_R, double* acc, int ld, int k0, float* deps, void* stream);
/* gacc[q] += (double)dc[q] for q < rows ncf (dc fp32 [rows][ncf] from the engine backward, gacc fp64).
 * hipErrorInvalidValue: a pointer null, rows or ncf < 1. */
int cdm_fit_grad_accum(const float* dc, int rows, int ncf, double* gacc, void* stream);
/* One pass of the fit closes here.  *done (device int) = passes completed; this is pass n = *done + 1 of iters + 1.
 * Per row r (score[r] = the accumulated objective, g = gacc[r][:]), all in fp64 with contraction off:
 *   gnorm = sqrt(sum over free columns j ascending of g[j] g[j]);  finite = isfinite(score) and every free g[j] finite
 *   hist_score[(n - 1) rows + r] = score;  hist_gnorm[(n - 1) rows + r] = gnorm
 *   score < best_score[r]:  best_score[r] = score, best_c[r][:] = c32[r][:] (the parameters the score was taken at)
 *   n <= iters and finite, per free column j (bc1 = bc[2 (n - 1)], bc2 = bc[2 (n - 1) + 1], the host-built
 *   1 - beta1^n and 1 - beta2^n):
 *     m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) (g g)
 *     c64 = clamp(c64 - (lr (m / bc1)) / (sqrt(v / bc2) + eps), lo[j], hi[j]);  c32 = (float)c64
 *   n <= iters and not finite:  stalled[r] += 1, the row's c64, c32, m, v keep their bits
 *   a column with free_mask[j] == 0 keeps its bits always; pass n = iters + 1 records and tracks the best only.
 * Then score and gacc are cleared, *pos_ctr (optional: the scan prologue's position counter) is reset to 0 and *done
 * becomes n.  *done outside 0..iters: nothing is read or written.  One block (a pass is rows ncf elements).
 * hipErrorInvalidValue, nothing launched: a required pointer null; iters, rows or ncf < 1. */
int cdm_fit_update(int* done, int iters, int rows, int ncf, double* score, double* gacc, const int* free_mask,
                   const double* lo, const double* hi, double lr, double beta1, double beta2, double eps, const double* bc,
                   double* c64, float* c32, double* m, double* v, double* best_score, float* best_c, double* hist_score,
                   double* hist_gnorm, int* stalled, int* pos_ctr, void* stream);
/* F.mse_loss + its gradient (code/train_diffusion_condition.py:227): loss = mean over the n elements, dpred =
 * 2 (pred - noise) / grad_numel (grad_numel = n, or the data-parallel count of a ragged global batch);
 * nonfinite (optional): += 1 when the loss is NaN / inf (SURVEY §5 failure guard; read once per epoch) */
int cdm_mse(const float* pred, const float* noise, long long n, double grad_numel, float* dpred, float* partial, int nb,
            float* loss_out, float* dbias_out, int* nonfinite, void* stream);
/* sampler.  One step of every sampler is: a prologue (below or cdm_sample_prologue_sub), the eval forward, one update
 * (cdm_denoise, cdm_ddim_step or cdm_dpmpp_step) and, in masked sampling, cdm_mask_blend.  The two prologues launch one
 * kernel; the update and blend kernels share the CFG combine eps = eu + w (ec - eu), the per-run key seed ^ *seed_dev
 * and the write-out (x, both halves of x2, the snapshot slot).
 * Ancestral prologue (device step counter; code/train_diffusion_condition.py:312-333): i = *ctr; *ctr = i - 1;
 * cur_i = i; t_cur = (float)((double)i / T); shortcut row T - i of sc_table.  A counter outside 1..T writes and reads
 * nothing.  cdm_denoise: denoise_add_noise + CFG combine (:274-279). */
int cdm_sample_prologue(int* ctr, int T, int* cur_i, float* t_cur, const float* sc_table, int sc_row, float* sc_cur,
                        void* stream);
/* z: z_table[(T - i) * zstride + e] when given, else Philox keyed by seed ^ *seed_dev (seed_dev optional: a
 * per-run device value, so one captured graph draws a fresh z sequence on every run) */
int cdm_denoise(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg, float w,
                const int* cur_i, const float* coef, const float* sa, const float* sb, const float* z_table,
                long long zstride, unsigned long long seed, const long long* seed_dev, const int* snap_slot,
                float* snaps, int T, void* stream);
/* strided (DDIM) sampler over the timestep subsequence steps[0..npos] (steps[0] = 0 < steps[1] < ... < steps[npos] = T;
 * the device counter holds the position k = npos..1).  Prologue: cur_k = k, cur_i = i = steps[k],
 * t_cur = (float)((double)i / T), *ctr = k - 1, shortcut row npos - k of sc_table.  A counter outside 1..npos writes
 * nothing (and the step kernel then does nothing either).  cdm_sample_prologue is this with npos = T and steps[k] = k. */
int cdm_sample_prologue_sub(int* ctr, int npos, int T, const int* steps, int* cur_i, int* cur_k, float* t_cur,
                            const float* sc_table, int sc_row, float* sc_cur, void* stream);
/* x <- (cx[k] x + ce[k] eps) + sigma[k] z with separate fp32 roundings; eps = eu + w (ec - eu) when cfg.  cx / ce /
 * sigma [npos + 1] are host-built tables indexed by the position k = *cur_k.  sigma[k] == 0: z is neither read nor
 * drawn; else z = z_table[(npos - k) * zstride + e] when given, else Philox keyed by seed ^ *seed_dev, stream
 * i = *cur_i (the timestep, as cdm_denoise).  Writes x (and both halves of x2 when given; x2 may alias x), and the
 * snapshot slot snap_slot[k] (snap_slot [npos + 1], optional) of snaps when >= 0. */
int cdm_ddim_step(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg, float w,
                  const int* cur_i, const int* cur_k, const float* cx, const float* ce, const float* sigma, int npos,
                  const float* z_table, long long zstride, unsigned long long seed, const long long* seed_dev,
                  const int* snap_slot, float* snaps, void* stream);
/* second-order multistep (DPM-Solver++ 2M) update at the position k = *cur_k of the same subsequence, with separate fp32
 * roundings in this order (eps = eu + w (ec - eu) when cfg):
 *   d = (x - sq[k] eps) * ra[k];  D = d when c1[k] == 0, else c0[k] d + c1[k] dprev;  x <- cx[k] x + cd[k] D;  dprev <- d
 * sq / ra / c0 / c1 / cx / cd [npos + 1] are host-built tables (sigma_i, 1 / alpha_i, the multistep weights, sigma_j /
 * sigma_i, alpha_j (1 - e^-h)).  dprev (numel floats, required) is written at every position and read only where
 * c1[k] != 0, so it may be uninitialised at the first position.  No z is read or drawn.  Writes x (and both halves of x2
 * when given; x2 may alias x), and the snapshot slot snap_slot[k] (snap_slot [npos + 1], optional) of snaps when >= 0.
 * A k outside 1..npos writes nothing.  hipErrorInvalidValue, nothing launched: a required pointer null, npos < 1,
 * numel < 0, snap_slot without snaps. */
int cdm_dpmpp_step(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg, float w,
                   const int* cur_k, const float* sq, const float* ra, const float* c0, const float* c1,
                   const float* cx, const float* cd, int npos, float* dprev, const int* snap_slot, float* snaps,
                   void* stream);
/* masked (inpainting) sampling: re-impose the known pixels on the state a step kernel (cdm_denoise, cdm_ddim_step,
 * cdm_dpmpp_step) has just written.  The step went from the timestep i = *cur_i to j: cur_k or steps null is the
 * ancestral form, position i of 1..T and j = i - 1; otherwise position k = *cur_k of 1..npos and j = steps[k - 1].
 * With separate fp32 roundings (m = mask[e % mask_numel], so a mask of numel / batch elements serves every sample):
 *   kn = sab[j] known + somab[j] xi  (j >= 1);  kn = known  (j == 0: xi neither read nor drawn, no multiply)
 *   x  = m kn + (1 - m) x            (m == 1 stores kn, m == 0 keeps x, bit for bit; known is not read where m == 0)
 * sab / somab [T + 1]: sqrt(ab) and sqrt(1 - ab) by timestep (diffusion.known_tables).  xi = row (fresh ? rows -
 * position : 0) of xi_table (rows = T or npos: the row order of the z tables) at stride xistride when given, else
 * Philox keyed by (seed ^ *seed_dev) ^ a fixed constant (a stream domain disjoint from z's), stream (fresh ? j : 0).
 * Writes x (and both halves of x2 when given; x2 may alias x) and the snapshot slot snap_slot[position] of snaps when
 * >= 0.  A position outside its range, or i outside 1..T, writes nothing.  hipErrorInvalidValue, nothing launched:
 * numel <= 0, mask_numel <= 0, numel % mask_numel != 0, a required pointer null, T < 1, npos outside 1..T in the strided
 * form, xistride < 0, snap_slot without snaps. */
int cdm_mask_blend(float* x, float* x2, long long numel, const float* known, const float* mask, long long mask_numel,
                   const int* cur_i, const int* cur_k, const int* steps, int npos, int T, const float* sab,
                   const float* somab, const float* xi_table, long long xistride, int fresh, unsigned long long seed,
                   const long long* seed_dev, const int* snap_slot, float* snaps, void* stream);
/* position programs (resampling, late start): a run of npos positions that may visit one timestep several times.  The
 * prologue is cdm_sample_prologue_sub with steps = the program's network timesteps (it reads only steps[k]), the update
 * cdm_ddim_step_pos or cdm_dpmpp_step with tables built per position, then cdm_mask_blend_jump.
 * cdm_ddim_step_pos is cdm_ddim_step with the device z keyed by the position: Philox under (seed ^ *seed_dev) ^ a fixed
 * constant of its own, stream k = *cur_k, so two visits to one timestep draw different z; the host z is row npos - k as
 * there.  hipErrorInvalidValue, nothing launched: a required pointer null, npos < 1, numel <= 0, zstride < 0, snap_slot
 * without snaps. */
int cdm_ddim_step_pos(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg, float w,
                      const int* cur_k, const float* cx, const float* ce, const float* sigma, int npos,
                      const float* z_table, long long zstride, unsigned long long seed, const long long* seed_dev,
                      const int* snap_slot, float* snaps, void* stream);
/* The blend of cdm_mask_blend at the level j = land_t[p] of the position p = *cur_k (land_t, fa, fb [npos + 1], by
 * position), then the forward jump, with separate fp32 roundings:
 *   v = the blend of x at j (cdm_mask_blend's arithmetic and m == 0 / m == 1 / j == 0 rules); mask null: v = x, and
 *       known / sab / somab are not read
 *   snapshot slot snap_slot[p] <- v
 *   x <- fa[p] v + fb[p] zeta  where fb[p] != 0, for every pixel, known ones included;  x <- v  where fb[p] == 0
 * xi: row (fresh ? npos - p : 0) of xi_table, else Philox in cdm_mask_blend's key domain, stream (fresh ? p : 0).
 * zeta: row npos - p of zeta_table at stride zetastride, else Philox keyed by (seed ^ *seed_dev) ^ a third constant,
 * stream p; neither read nor drawn where fb[p] == 0.  Writes x (and both halves of x2 when given; x2 may alias x).  A p
 * outside 1..npos, or a j outside 0..T, writes nothing.  hipErrorInvalidValue, nothing launched: numel <= 0, x / cur_k /
 * land_t / fa / fb null, npos < 1, T < 1, a negative stride, snap_slot without snaps, and with a mask: known / sab /
 * somab null, mask_numel <= 0, numel % mask_numel != 0. */
int cdm_mask_blend_jump(float* x, float* x2, long long numel, const float* known, const float* mask, long long mask_numel,
                        const int* cur_k, const int* land_t, int npos, int T, const float* sab, const float* somab,
                        const float* fa, const float* fb, const float* xi_table, long long xistride, int fresh,
                        const float* zeta_table, long long zetastride, unsigned long long seed,
                        const long long* seed_dev, const int* snap_slot, float* snaps, void* stream);
/* Observation-guided sampling (diffusion.GuidedDDIMSampler, not in the reference; csrc/guide.hip): diffusion posterior
 * sampling against y = A x0 + n, A the f x f block mean [H, H] -> [H / f, H / f], with a per-cell weight.  A step is
 * cdm_sample_prologue_sub, the frozen train-structured forward, cdm_obs_residual_grad, the engine's full backward with
 * dx, and cdm_ddim_step_guided.  Neither kernel synchronises or allocates.
 * cdm_obs_residual_grad, at the position p = *cur_k (sq / ra [npos + 1]: sqrt(1 - ab_i) and 1 / sqrt(ab_i) by position,
 * diffusion.guided_tables), each line one fp32 rounding unless marked (eps = eu + w (ec - eu) when cfg):
 *   x0h_e = (x_e - sq[p] eps_e) * ra[p]
 *   m_q   = (the f f x0h of cell q added in row-major order) * (1 / f^2);   r_q = obs_q - m_q
 *   L[s]  = sum_q ((double)wgt_q (double)r_q) (double)r_q    fp64, assigned; hist[p n + s] = L[s]  (hist [npos + 1][n])
 *   u_e   = (wgt_q r_q) * (1 / f^2) for every pixel e of cell q
 *   gdir_e = (float)(-2 (double)ra[p]) u_e;   ge_e = (float)(2 (double)sq[p] (double)ra[p]) u_e
 *   deps_e = ge_e;  with cfg: w ge_e on the cond row, (1 - w) ge_e on the uncond row (deps [n or 2 n][H H])
 * x [n][H][H], eps [n or 2 n][H][H], obs [n][H / f][H / f]; wgt_q = wgt[(s cells + q) % wgt_numel], so a weight plane of
 * one sample serves the batch.  A cell with wgt_q == 0 is not observed: obs_q is not read, u = 0, nothing added to L.
 * One block per sample, one thread owns whole cells; per-thread fp64 sums over a fixed cell set (q = t, t + 256, ...),
 * a wave64 butterfly, a fixed-order fold of the four wave sums through LDS: two runs give the same bits; no atomics.
 * deps and gdir both null: only L and hist are written (the zeta == 0 form).  A p outside 1..npos writes nothing.
 * hipErrorInvalidValue, nothing launched: a required pointer null; n, H or npos < 1; f not in {1, 2, 4, 8}; H % f != 0;
 * wgt_numel neither the cell count nor n times it; exactly one of deps and gdir null. */
int cdm_obs_residual_grad(const float* x, const float* eps, int cfg, float w, const float* obs, const float* wgt,
                          long long wgt_numel, int n, int H, int f, const int* cur_k, const float* sq, const float* ra,
                          int npos, double* L, double* hist, float* deps, float* gdir, void* stream);
/* cdm_ddim_step_pos (its update, position-keyed z, host-z row and write-out) followed by a step of length zeta down the
 * gradient of the misfit norm sqrt(L), with separate fp32 roundings (s = e / H^2, the sample):
 *   grad_e = (grad_dir_e + dx_e) (+ dx_{numel + e} when cfg)
 *   k_s    = (float)((double)zeta / (2 sqrt(L[s])));   x <- ((cx[k] x + ce[k] eps) + sigma[k] z) - k_s grad_e
 * Where L[s] == 0, and everywhere when zeta == 0, nothing is subtracted and x has cdm_ddim_step_pos's bits; with
 * zeta == 0 grad_dir, dx and L are not read and may be null.  dx [numel or 2 numel]: the engine backward's image
 * gradient.  hipErrorInvalidValue, nothing launched: what cdm_ddim_step_pos rejects; H < 1; numel % H^2 != 0; zeta
 * negative or not finite; zeta > 0 with grad_dir, dx or L null. */
int cdm_ddim_step_guided(const float* xin, float* x, float* x2, long long numel, const float* eps, int cfg, float w,
                         const int* cur_k, const float* cx, const float* ce, const float* sigma, int npos,
                         const float* z_table, long long zstride, unsigned long long seed, const long long* seed_dev,
                         const int* snap_slot, float* snaps, const float* grad_dir, const float* dx, const double* L,
                         float zeta, int H, void* stream);
/* Flow likelihood (diffusion.FlowLikelihood, not in the reference; csrc/flow.hip): the log-density of the eta = 0 DDIM
 * sampler's model by the change of variables along the ascending (encoding) walk x -> ix[p] x + ie[p] eps(x), whose
 * Jacobian is ix[p] (I + g[p] J), J = d eps / d x.  A step is cdm_sample_prologue_sub (steps = the ascending timesteps
 * by position), the frozen train-structured forward, cdm_flow_probe into deps, the engine's full backward with dx
 * (dx = J^T v), and cdm_flow_step.  No kernel synchronises or allocates; the position p = *cur_k is read from the device
 * and a p outside 1..npos writes nothing.  No timing of these kernels has been taken.
 * cdm_flow_probe: the Rademacher probe v [n][H][H], v[b][e] = u[e] < 0.5f ? 1 : -1 with u what
 * cdm_philox_uniform(out, H H, 0, 1, key, sub = p) writes, key = (seed ^ *seed_dev) ^ a fixed constant of its own
 * (seed_dev optional).  Keyed by the position and the element within the map, not by the row: all rows of a run share
 * their probes (common random numbers), two run keys give different ones.  hipErrorInvalidValue, nothing launched: v or
 * cur_k null; n, H or npos < 1.
 * cdm_flow_step, one block of 256 threads per row, v regenerated from the same key (the buffer the backward was handed
 * is not read), ix / ie fp32 and g fp64 tables [npos + 1] by position (diffusion.encode_tables), D = H H:
 *   q       = sum_e (double)dx[e] (double)v[e]     fp64: thread t adds e = t, t + 256, ... ascending, a wave64 butterfly,
 *                                                  then (w0 + w1) + (w2 + w3) through LDS: the same bits every run
 *   form 0 (trace):   ld = g[p] q
 *   form 1 (logdet):  a = (g[p] q) / D;  ld = D log1p(a) where a > -1, else NaN
 *   acc[row] += ld;   hist[p n + row] = q  (hist [npos + 1][n]);   invalid[row] = 1 where ld is not finite
 *   x[e] <- ix[p] x[e] + ie[p] eps[e]              fp32: two products and one sum, each one rounding
 * Every fp64 line is one rounding too; log1p is evaluated from IEEE operations alone (frexp, an atanh series of twelve
 * terms by Horner; the kernel's comment has every line), so a host restatement reproduces acc bit for bit.  x, eps, dx
 * [n][H][H]; there is no CFG form.  hipErrorInvalidValue, nothing launched: a pointer null; n, H or npos < 1; form not
 * 0 or 1.
 * cdm_flow_finish, per row, the same summation order: ss = sum_e (double)x[e]^2; prior[row] = -0.5 ss - (0.5 D) log(2 pi)
 * (log N(x_T; 0, I)); logp[row] = (prior[row] + (0.5 D) log_abT) + acc[row].  hipErrorInvalidValue, nothing launched: a
 * pointer null; n or H < 1; log_abT not finite or > 0. */
int cdm_flow_probe(float* v, int n, int H, const int* cur_k, int npos, unsigned long long seed, const long long* seed_dev,
                   void* stream);
int cdm_flow_step(float* x, const float* eps, const float* dx, int n, int H, const int* cur_k, const float* ix,
                  const float* ie, const double* g, int npos, int form, unsigned long long seed,
                  const long long* seed_dev, double* acc, double* hist, int* invalid, void* stream);
int cdm_flow_finish(const float* x, int n, int H, double log_abT, const double* acc, double* prior, double* logp,
                    void* stream);
/* randn_like/ randint / the per-forward random 1x1 shortcut draw (diffusion_utilities.py:54), on-device Philox.
 * The stream id is sub (+ *sub_dev when given, mod 2^32: a device counter advanced by cdm_counter_add, so a captured
 * step draws fresh numbers on every replay).  Callers that give each consumer the sub-stream k << 24 plus a step
 * counter keep their streams disjoint for fewer than 2^24 steps.
 * The contract of every device draw (csrc/sampler_parts.h; tests/_rng_ref.py restates it on the host and
 * tests/test_gpu_rng.py holds the device to it):
 *   words   Philox4x32-10 (Random123's multipliers, key schedule and word order) under the key words
 *           ((uint32)seed, seed >> 32), of the counter (c0, c1, c2, c3) with c3 the domain word:
 *             0x5EED  normal:  (q, q >> 32, sub, 0x5EED); element 4 q + 0 / 1 = r cos / r sin of the words (x, y),
 *                      4 q + 2 / 3 of (z, w); r = sqrtf(-2 logf(u1)), angle 6.283185307179586f * u2, (u1, u2) = u01 of
 *                      the pair.  cdm_philox_normal and every in-kernel z / xi / zeta.
 *             0x0417  uniform: (q, q >> 32, sub, 0x0417); element 4 q + j = lo + (hi - lo) u01(word j) in fp32 (the
 *                      product and the sum may be one fma; at (0, 1) it is u01 itself).  cdm_philox_uniform,
 *                      cdm_context_drop, cdm_augment_draw, cdm_tsample_draw, cdm_flow_probe.
 *             0xA11C  randint: (i, 0x71, sub, 0xA11C); element i = lo + (((x << 32) | y) % (hi - lo + 1)).
 *   u01(v) = ((float)(v >> 8) + 0.5f) * 2^-24 in fp32.  Range (0, 1], not (0, 1): for v >> 8 >= 2^23 the + 0.5f is a
 *           tie and rounds to even, so v >> 8 == 0xFFFFFF gives exactly 1.0f (and the upper half of the range has half
 *           the resolution).  Never 0: the smallest value is 2^-25.  cdm_philox_uniform(out, 1, 0, 1, 0, 1543363)
 *           writes 1.0f.
 *   keys    the samplers' draws are keyed by seed ^ *seed_dev, XOR one of four key-domain constants, each the big-endian
 *           ASCII of its name and nothing else:
 *             (none)                                   z of cdm_denoise and cdm_ddim_step, stream i (the timestep)
 *             0x706F735F73746570 "pos_step"  STEP_NOISE_DOMAIN   z of cdm_ddim_step_pos / _guided, stream k
 *             0x6B6E6F776E5F7869 "known_xi"  KNOWN_NOISE_DOMAIN  xi of cdm_mask_blend (stream fresh ? j : 0) and
 *                                                                of cdm_mask_blend_jump (stream fresh ? p : 0)
 *             0x6A756D707A657461 "jumpzeta"  JUMP_NOISE_DOMAIN   zeta of cdm_mask_blend_jump, stream p
 *             0x666C6F7770726F62 "flowprob"  FLOW_PROBE_DOMAIN   the probes of cdm_flow_probe / cdm_flow_step, stream p
 * hipErrorInvalidValue, nothing launched: n < 0; out null with n > 0; cdm_philox_uniform with lo or hi not finite or
 * hi < lo; cdm_philox_randint with hi < lo or hi - lo + 1 beyond an int.  n == 0 returns 0 without a launch. */
int cdm_philox_normal(float* out, long long n, unsigned long long seed, unsigned int sub, const int* sub_dev,
                      void* stream);
int cdm_philox_uniform(float* out, long long n, float lo, float hi, unsigned long long seed, unsigned int sub,
                       const int* sub_dev, void* stream);
int cdm_philox_randint(int* out, int n, int lo, int hi, unsigned long long seed, unsigned int sub, const int* sub_dev,
                       void* stream);
int cdm_counter_add(int* ctr, int delta, void* stream);
/* torch.optim.Adam step (code/train_diffusion_condition.py:200,229) with torch's CPU roundings.
 * state (double[4], device) = {lr, step count, scratch, scratch}; bc (double[nbc][2], device) = host-evaluated
 * {1 - beta1**s, (1 - beta2**s)**0.5} for s = 1..nbc (steps past nbc reuse the last row, which must be {1, 1}).
 * grad_scale multiplies g (1/world for a summed data-parallel gradient). */
int cdm_adam(float* p, const float* g, float* m, float* v, long long n, double* state, const double* bc, int nbc,
             double beta1, double beta2, double eps, float grad_scale, void* stream);
/* cdm_adam plus the exponential moving average of the parameters in the same pass: p, m, v and state come out
 * bit-identical to cdm_adam; then ema[i] = fmaf(omd, p_new - ema[i], ema[i]) with omd = (float)(1 - *ema_decay)
 * (*ema_decay == 0: ema[i] = p_new exactly).  ema_decay is a device double[1], read at run time like lr in state, so
 * it can change between replays of a captured step.  hipErrorInvalidValue, nothing launched: nbc < 1, n < 0, ema or
 * ema_decay null.  n == 0 advances the step count only. */
int cdm_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, double* state, const double* bc,
                 int nbc, double beta1, double beta2, double eps, float grad_scale, const double* ema_decay,
                 void* stream);
/* Global-norm gradient clipping and the non-finite step skip (torch.nn.utils.clip_grad_norm_ in front of
 * optim.step()), computed on the device so a captured step needs no host read.
 * cdm_grad_sumsq: partial[b] = sum over block b's elements of (double)g[i] * (double)g[i], b < nb, plain stores.
 * nb = clamp(ceil(n / 4096), 1, CDM_GRAD_SUMSQ_MAX_PARTIALS), a function of n alone; *nb_out (optional, a host int)
 * receives it.  Every thread sums a fixed set of elements in fp64 and the wave / block folds have a fixed order: the
 * partials, and any fixed-order sum of them, are the same bits in every run.  g needs 4-byte alignment only (a slice
 * of a larger buffer): the elements before the first 16-byte boundary and after the last whole float4 are read one by
 * one, the rest as float4.  n == 0 writes partial[0] = 0.  hipErrorInvalidValue, nothing launched: partial null,
 * n < 0, g null with n > 0, g not 4-byte aligned. */
#define CDM_GRAD_SUMSQ_MAX_PARTIALS 2048
int cdm_grad_sumsq(const float* g, long long n, double* partial, int* nb_out, void* stream);
/* cdm_adam / cdm_adam_ema behind that guard, three launches: cdm_grad_sumsq's kernel into partial (caller-owned,
 * room for cdm_grad_sumsq's nb doubles; CDM_GRAD_SUMSQ_MAX_PARTIALS always suffices), one block that sums the
 * partials in a fixed order to S and writes clip_rec (device double[3]) = {norm, coef, skip}:
 *   norm = sqrt(S) * grad_scale                            fp64: the norm of the gradient Adam sees
 *   skip = !isfinite(S)                                    1.0 / 0.0; S is non-finite exactly when an element of g is
 *   coef = (float)min(1.0, *max_norm / (norm + 1e-6))      max_norm: device double[1] read at run time, like lr in
 *                                                          state; +inf gives coef == 1 exactly
 * and, if skip, adds 1 to *skipped (device int) and leaves state alone, otherwise advances state as cdm_adam does;
 * then the Adam kernel with gi = (g[i] * grad_scale) * coef, two fp32 roundings, every other expression cdm_adam's
 * (and cdm_adam_ema's for the EMA): at coef == 1 the results are cdm_adam's bits, at coef < 1 those of cdm_adam on
 * the gradient (g * grad_scale) * coef with grad_scale 1.  If skip, the kernel returns before it reads or writes p, m,
 * v, ema: parameters, moments, step count and EMA are untouched.  ema and ema_decay are optional, both or neither.
 * n == 0: norm 0, coef 1, no skip, the step count advances, nothing else.  hipErrorInvalidValue, nothing launched:
 * p, g, m, v, state, bc, max_norm, partial, clip_rec or skipped null; n < 0; nbc < 1; ema without ema_decay or
 * ema_decay without ema; g not 4-byte aligned. */
int cdm_adam_clipped(float* p, const float* g, float* m, float* v, float* ema, long long n, double* state,
                     const double* bc, int nbc, double beta1, double beta2, double eps, float grad_scale,
                     const double* ema_decay, const double* max_norm, double* partial, double* clip_rec, int* skipped,
                     void* stream);
/* context dropout (training for classifier-free guidance): u[b] = element b of what
 * cdm_philox_uniform(out, B, 0, 1, seed, sub, sub_dev) writes; c_out[b][:] = u[b] < p_drop ? 0 : c[b][:] for c, c_out
 * [B][ncf]; keep (optional, int [B]) = 0 where the row was dropped, else 1.  c_out must not be c.  u lies in (0, 1]
 * (u01 reaches 1.0f), so p_drop == 1 is a case of its own: it drops every row, whatever u.  Every p_drop < 1 is the
 * plain comparison, so p_drop = 0.99999994f keeps a row whose u is 1.0f.
 * hipErrorInvalidValue: p_drop outside [0, 1] or NaN, B < 1, ncf < 1, c or c_out null, c_out == c. */
int cdm_context_drop(const float* c, int B, int ncf, float p_drop, unsigned long long seed, unsigned int sub,
                     const int* sub_dev, float* c_out, int* keep, void* stream);
/* symmetry augmentation of square single-channel maps (Trainer(augment=...)).  An op is {g, dy, dx}: f = g >> 2 flips
 * the columns, then r = g & 3 quarter turns, then a periodic roll by (dy, dx) rows / columns, i.e. on one [H][H] map
 *     x = x.flip(-1) if f else x;  x = torch.rot90(x, r, (-2, -1));  x = torch.roll(x, (dy, dx), (-2, -1)).
 * Output pixel (i, j) is input pixel (i', j'); with n = H - 1, a = (i - dy) mod H, b = (j - dx) mod H:
 *     g   0   1      2      3      4      5   6      7
 *     i'  a   b      n - a  n - b  a      b   n - a  n - b
 *     j'  b   n - a  n - b  a      n - b  a   b      n - a
 * cdm_augment_draw: ops [B][3].  u = elements 3b, 3b + 1, 3b + 2 of what cdm_philox_uniform(out, 3 B, 0, 1, seed, sub,
 * sub_dev) writes; g = min(7, (int)(8 u0)), dy = min(H - 1, (int)(H u1)), dx = min(H - 1, (int)(H u2)), in fp32.
 * mode: 0 none, 1 d4 (g drawn), 2 shift (dy, dx drawn), 3 both; what the mode does not draw is 0, and every mode
 * consumes all three uniforms.  hipErrorInvalidValue: ops null, B < 1, H < 1, mode outside 0..3. */
int cdm_augment_draw(int* ops, int B, int H, int mode, unsigned long long seed, unsigned int sub, const int* sub_dev,
                     void* stream);
/* cdm_perturb with the gather folded in: out[b][p] = sab[t_b] x[b][src_b(p)] + omab[t_b] noise[b][p] (+ tin), the same
 * fp32 expression and roundings as cdm_perturb (all-zero ops: its output bit for bit); the noise is not transformed and
 * there is no intermediate buffer.  noise == NULL: out[b][p] = x[b][src_b(p)] alone (t, cur_i, sab, omab, tin unused).
 * An op outside its range is clamped into it (callers validate on the host).  hipErrorInvalidValue: x, ops or out
 * null; out == x; N < 1; H < 1; HW != H * H; with noise: neither t nor cur_i, sab or omab null, T < 1. */
int cdm_perturb_aug(const float* x, const int* ops, const float* noise, const int* t, const int* cur_i,
                    long long nstride, const float* sab, const float* omab, int N, int HW, int H, int T, float* out,
                    float* tin, void* stream);
/* Timestep-aware training loss (Trainer(loss_weight=..., t_sampler=..., t_record=...), not in the reference;
 * csrc/tloss.hip).  The timesteps 1..T fall into NB <= CDM_TLOSS_MAX_BUCKETS buckets: edge_k = (k T) / NB
 * in integer arithmetic for k = 0..NB, bucket k = edge_k + 1 .. edge_{k+1}, n_k = edge_{k+1} - edge_k >= 1 (NB <= T);
 * the bucket of t is (t NB - 1) / T.  None of the three synchronises or allocates.
 * cdm_tsample_draw: t [B] int and iw [B] fp32 from cdf [NB] fp64 and iw_tab [NB] fp32.  u0, u1 = elements 2b, 2b + 1
 * of what cdm_philox_uniform(out, 2 B, 0, 1, seed, sub, sub_dev) writes; k = the count of j in 0..NB-2 with
 * cdf[j] <= (double)u0 (cdf[NB - 1] is never read: a u0 of exactly 1 lands in bucket NB - 1);
 * t[b] = edge_k + 1 + min(n_k - 1, (int)((float)n_k * u1)) in fp32; iw[b] = iw_tab[k].
 * hipErrorInvalidValue, nothing launched: a pointer (other than sub_dev) null; B, T or NB < 1; NB > T;
 * NB > CDM_TLOSS_MAX_BUCKETS. */
#define CDM_TLOSS_MAX_BUCKETS 1024
int cdm_tsample_draw(int* t, float* iw, int B, int T, int NB, const double* cdf, const float* iw_tab,
                     unsigned long long seed, unsigned int sub, const int* sub_dev, void* stream);
/* cdm_mse with a weight per row: pred, noise, dpred [B][HW]; omega_b = w_tab[t[b]] * iw[b], one fp32 product (w_tab
 * [T + 1] fp32 and iw [B] fp32 may each be null and then count as 1; t [B] int is read only with w_tab, and t[b] must
 * index it: the call cannot check that);
 *   d = pred - noise                                  fp32
 *   dpred[b][p] = d * ((float)(2 / grad_numel) * omega_b)      the factor one fp32 product; both tables null: the factor
 *                                                     is (float)(2 / grad_numel) and dpred has cdm_mse's bits
 *   row_sq[b] = sum_p (double)d (double)d,  row_g[b] = sum_p (double)dpred[b][p]       fp64 [B] each
 *   loss = (float)((sum_b (double)omega_b * row_sq[b]) / ((double)B * (double)HW)),  dbias = (float)(sum_b row_g[b])
 * the last two by one thread over b = 0..B-1 in order, one IEEE fp64 operation per step; nonfinite (optional) += 1
 * when the loss is NaN / inf.  One block of 256 threads per row; any HW >= 1 and 4-byte aligned bases: float4 loads /
 * stores on the 16-byte aligned body of a row when the three rows agree mod 16, scalar head and tail; per-thread fp64
 * sums over a fixed element set, a wave64 butterfly, a fixed-order fold: two runs give the same bits; no atomics.
 * hipErrorInvalidValue, nothing launched: pred, noise, dpred, row_sq or row_g null; w_tab without t; B or HW < 1;
 * grad_numel <= 0. */
int cdm_mse_weighted(const float* pred, const float* noise, int B, int HW, const int* t, const float* w_tab,
                     const float* iw, double grad_numel, float* dpred, double* row_sq, double* row_g, float* loss_out,
                     float* dbias_out, int* nonfinite, void* stream);
/* The per-bucket record of the raw loss and the loss-aware timestep table.  rec [NB][3] fp64 = {n, m1, m2}: samples
 * seen, EMA of l, EMA of y = (w_tab[t] l)^2 (w_tab null: l^2; the importance weight is not part of it).  One thread,
 * for b = 0..B-1 in order, every fp64 operation one IEEE operation (no contraction):
 *   l = row_sq[b] / (double)HW;  a non-finite l, or a t[b] outside 1..T, leaves the record alone
 *   k = bucket of t[b];  wl = (double)w_tab[t[b]] * l;  y = wl * wl
 *   n == 0:  m1 = l, m2 = y;   else  m1 = m1 + alpha * (l - m1),  m2 = m2 + alpha * (y - m2);   then n = n + 1
 * mode 0 stops here (cdf, iw_tab unread and unwritten: they may be null).  mode 1 rebuilds cdf [NB] fp64 and iw_tab
 * [NB] fp32 from the record alone: S = the in-order sum of sqrt(m2_k);
 *   uniform form, while min_k n < warmup, or S is not finite or not > 0:
 *     cdf[k] = (double)edge_{k+1} / (double)T,  iw_tab[k] = 1.0f
 *   else  q_k = ((1 - mix) * sqrt(m2_k)) / S + (mix * n_k) / T;  cdf[k] = the in-order running sum of q;
 *     iw_tab[k] = (float)(n_k / (T * q_k))        (n_k here the bucket's size, T and n_k as doubles)
 * hipErrorInvalidValue, nothing launched: row_sq, t or rec null; B, HW, T or NB < 1; NB > T;
 * NB > CDM_TLOSS_MAX_BUCKETS; alpha outside (0, 1]; mode outside 0..1; mode 1 with cdf or iw_tab null, warmup < 1 or
 * mix outside (0, 1]. */
int cdm_tloss_record(const double* row_sq, const int* t, const float* w_tab, int B, int HW, int T, int NB, double alpha,
                     double* rec, int mode, int warmup, double mix, double* cdf, float* iw_tab, void* stream);
/* weight repacking (+ eval-mode BatchNorm folding) */
/* kc = 0: K order tap-major (k = tap*C + ci); kc = 16: channel-chunk-major (k = ((ci/16)*9 + tap)*16 + ci%16),
 * the order cdm_conv3x3_fwd(kc = 16) consumes (wdg is chunked over Cout).  ConvTranspose packing: */
int cdm_pack_conv3x3(const float* W, const float* b, int Cin, int Cout, const float* gamma, const float* beta,
                     const float* rm, const float* rv, float eps, float* wpk, float* bpk, float* wdg, int kc,
                     void* stream);
int cdm_pack_convT(const float* W, int Cin, int Cout, int KK, float* wt, float* wtT, void* stream);
int cdm_transpose(const float* in, int R, int C, float* out, void* stream);
/* batched: in [batch][R][C] -> out [batch][C][R] (64x64 LDS tiles) */
int cdm_transpose_batched(const float* in, int batch, int R, int C, float* out, void* stream);

/* up0 on large maps (ContextUnet.py:26-27, ConvTranspose2d(C, C, k, k) on the 1x1 to_vec map, KK = k*k), VALU fp32
 * kernels over the weights in the reference layout W[ci][co][KK] (no repack): forward y[n][KK][C] (NHWC) =
 * bias + x[n][:] W (any B >= 1, one read of W per 16 samples); weight gradient dW[ci][co][KK] = x^T dy with
 * dy [B][KK][C] (NHWC), B <= 16 (assigns).  C % 16 == 0, C <= 512, KK % 64 == 0 (weight gradient: KK % 256 == 0). */
int cdm_up0_fwd(const float* x, int B, int C, const float* W, int KK, const float* bias, float* y, void* stream);
int cdm_up0_wgrad(const float* x, int B, int C, const float* dy, int KK, float* dW, void* stream);
/* input gradient dx[n][ci] = sum_k dyT[n][k] W[ci][k] over k = (co, ij), dyT = dy transposed per sample to [B][C][KK]
 * (B <= 16, C % 64 == 0): per-K-range partials slab [cdm_up0_dgrad_splits(C, KK)][B][C], folded by cdm_slab_reduce */
int cdm_up0_dgrad(const float* dyT, int B, int C, const float* W, int KK, float* slab, void* stream);
int cdm_up0_dgrad_splits(int C, int KK);

#ifdef __cplusplus
}
#endif
#endif /* CDM_HIP_H */
