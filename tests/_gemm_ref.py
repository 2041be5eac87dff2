"""fp64 CPU references, exact-data generators, restated dispatch predicates and the case lists for the contraction code
of csrc/gemm_f32.hip and the kernels its launchers pick from csrc/conv_kernels.h: the ConvT 2x2 forward / input gradient
/ weight gradient (fp32, h3 and one-term bf16; the two-deep prefetch kernel and the transposed-read weight gradient), the
fp32 3x3 conv with its split-bf16 siblings, the dense GEMMs and the slab reduce.  Shared by tests/test_gpu_gemm_ops.py,
which holds the kernels to them, and tests/test_gemm_refs_cpu.py, which holds these functions to torch's fp64 operators
and checks, for every listed case, the conditions under which bit-equality is the right bar and that the data can see the
errors the cases are about.

Layouts: activations NHWC fp64 numpy arrays, ConvT weights [Cin][Cout][2][2], 3x3 weights OIHW.  The exact-data method
and its helpers are tests/_conv_ref.py's.  Operands are integer multiples of 2^-3 in [-1, 1] drawn independently (both
signs, no symmetry: a swapped sub-pixel, tap or transposed index changes the result), with one element of every operand
forced to +-1, so that cdm_amax_f32 gives 1 and the h3 operand scale is 2^13 whatever the draw.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _conv_ref import (EPI_ACCUM, EPI_RELU, NT_H3, SENT, _seed, bf16, budget, cached, chain_bound, check,  # noqa: F401
                       conv3x3, conv3x3_dgrad, conv3x3_wgrad, d3, effective_splits, epilogue, exact, f32, fits16,
                       fp32_exact, gauss, pick, tile_stats)

GBM = GBN = 128      # block tile of every GEMM kernel here (csrc/conv_kernels.h)
BK = 16              # K tile
SCALES = (1.0, 0.5, -2.0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


# ----------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------
def operand(rng, shape, exact_data=True, scale=1.0):
    """exact: multiples of 2^-3 in [-1, 1], one element forced to +-1 (max|.| = 1); else Gaussian fp32 values"""
    if not exact_data:
        return gauss(rng, shape, scale)
    a = d3(rng, shape)
    p, q = (int(v) for v in rng.choice(a.size, 2, replace=False))
    s = float(pick(rng, (), [1.0, -1.0]))
    a.reshape(-1)[p] = s                                             # max|a| = 1 ...
    a.reshape(-1)[q] = -s * float(rng.integers(1, 9)) * 2.0 ** -3    # ... and both signs, whatever the draw
    return a


def q16(a, ops):
    """the operand as the one-term arithmetic sees it (ops = 1: rounded to bf16)"""
    return bf16(a) if ops else a


# ----------------------------------------------------------------------------------------------------------------
# split-K ranges (launch_gemm / effective_splits restated)
# ----------------------------------------------------------------------------------------------------------------
def split_ranges(K, splits, shift=None):
    """[(k0, k1)] per non-empty split: ktiles = ceil(K / 16), per = ceil(ktiles / splits), split z owns K tiles
    [z per, min(ktiles, (z + 1) per)).  shift = z: that split's range moved up by one tile (a wrong emulation for
    the sensitivity checks)"""
    kt = (K + BK - 1) // BK
    sp = min(max(1, splits), max(kt, 1))
    per = (kt + sp - 1) // sp
    out = []
    for z in range((kt + per - 1) // per if kt else 1):
        t0, t1 = z * per, min(kt, (z + 1) * per)
        if shift == z:
            t0, t1 = min(kt, t0 + 1), min(kt, t1 + 1)
        out.append((min(K, t0 * BK), min(K, t1 * BK)))
    assert len(out) == effective_splits(K, splits)
    return out


# ----------------------------------------------------------------------------------------------------------------
# ConvTranspose2d(Cin, Cout, 2, 2)
# ----------------------------------------------------------------------------------------------------------------
def convT_fwd(x, Wt, b=None):
    """y[n, 2h + i, 2w + j, co] = b[co] + sum_ci x[n, h, w, ci] W[ci][co][i][j]"""
    N, H, W, _ = x.shape
    y = np.einsum("nhwc,cdij->nhiwjd", x, Wt).reshape(N, 2 * H, 2 * W, Wt.shape[1])
    return y if b is None else y + b


def convT_dgrad(dy, Wt):
    """dx[n, h, w, ci] = sum_{i, j, co} dy[n, 2h + i, 2w + j, co] W[ci][co][i][j]"""
    N, H2, W2, Co = dy.shape
    return np.einsum("nhiwjd,cdij->nhwc", dy.reshape(N, H2 // 2, 2, W2 // 2, 2, Co), Wt)


def _convT_cols(dy):
    """dy [N, 2H, 2W, Co] -> [input pixel (n, h, w)][ij Co + co], the B operand of the weight-gradient GEMM"""
    N, H2, W2, Co = dy.shape
    return dy.reshape(N, H2 // 2, 2, W2 // 2, 2, Co).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4 * Co)


def convT_wgrad_parts(x, dy, splits, shift=None):
    """[sp][Cin][ij Cout + co]: the partial of each split's input-pixel range (the slab of cdm_convT2x2_wgrad)"""
    X, D = x.reshape(-1, x.shape[-1]), _convT_cols(dy)
    return np.stack([X[k0:k1].T @ D[k0:k1] for k0, k1 in split_ranges(X.shape[0], splits, shift)])


def convT_wgrad(x, dy):
    """dW[ci][co][i][j] = sum_{n, h, w} x[n, h, w, ci] dy[n, 2h + i, 2w + j, co]"""
    Ci, Co = x.shape[-1], dy.shape[-1]
    return convT_wgrad_parts(x, dy, 1)[0].reshape(Ci, 2, 2, Co).transpose(0, 3, 1, 2)


def convT_pack(Wt):
    """wpk [Cin][ij Cout + co] (cdm_pack_convT's wt; wtT is its transpose)"""
    Ci, Co = Wt.shape[:2]
    return Wt.transpose(0, 2, 3, 1).reshape(Ci, 4 * Co)


# ----------------------------------------------------------------------------------------------------------------
# 3x3 conv weight gradient with its split partials (slab [z][co][tap Cin + ci])
# ----------------------------------------------------------------------------------------------------------------
def conv3x3_wgrad_parts(gy, x, splits, shift=None):
    N, H, W, Ci = x.shape
    xp = np.zeros((N, H + 2, W + 2, Ci))
    xp[:, 1:-1, 1:-1] = x
    cols = np.concatenate([xp[:, ky:ky + H, kx:kx + W].reshape(-1, Ci) for ky in range(3) for kx in range(3)], axis=1)
    G = gy.reshape(-1, gy.shape[-1])
    return np.stack([G[k0:k1].T @ cols[k0:k1] for k0, k1 in split_ranges(G.shape[0], splits, shift)])


def slab_to_oihw(part, Cin):
    """[co][tap Cin + ci] -> OIHW"""
    return part.reshape(part.shape[0], 3, 3, Cin).transpose(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------------------------------
# dense GEMMs
# ----------------------------------------------------------------------------------------------------------------
def gemm(a, b, bias=None, bias_mod=1, flags=0, old=None, wrong_bias=False):
    """C = A B + bias[n % bias_mod], then the epilogue flags.  wrong_bias: bias indexed by n (zeros past its end)"""
    v = a @ b
    if bias is not None:
        n = np.arange(b.shape[1])
        v = v + (np.concatenate([bias[:bias_mod], np.zeros(b.shape[1])])[n] if wrong_bias else bias[n % bias_mod])
    return epilogue(v, flags, old)


def gemm_parts(a, b, splits, shift=None):
    return np.stack([a[:, k0:k1] @ b[k0:k1] for k0, k1 in split_ranges(a.shape[1], splits, shift)])


def gemm_tn_parts(a, b, splits, shift=None):
    """a [K][M], b [K][N] -> [sp][M][N] partials of A^T B"""
    return np.stack([a[k0:k1].T @ b[k0:k1] for k0, k1 in split_ranges(a.shape[0], splits, shift)])


# ----------------------------------------------------------------------------------------------------------------
# slab reduce
# ----------------------------------------------------------------------------------------------------------------
def slab_index(M, N, s_m, s_hi, s_lo, csplit):
    cs = csplit if csplit > 0 else N
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    return m * s_m + (n // cs) * s_hi + (n % cs) * s_lo


def slab_reduce(slab, out_old, s_m, s_hi, s_lo, csplit, accumulate, scale, strict=True):
    """out[m s_m + (n / csplit) s_hi + (n % csplit) s_lo] (+)= scale sum_z slab[z][m][n] on a copy of the flat buffer
    out_old (csplit = 0: N); elements no (m, n) maps to keep their old value.  strict = False (wrong emulations only):
    addresses may collide (the last one wins) and wrap at the end of the buffer"""
    _, M, N = slab.shape
    idx = slab_index(M, N, s_m, s_hi, s_lo, csplit)
    out = np.array(out_old, dtype=np.float64).reshape(-1).copy()
    if strict:
        assert np.unique(idx).size == idx.size and idx.max() < out.size, "not a permutation into the buffer"
    else:
        idx = idx % out.size
    v = scale * slab.sum(0)
    out[idx] = (out[idx] + v) if accumulate else v
    return out


# ----------------------------------------------------------------------------------------------------------------
# the launchers' dispatch predicates, restated (csrc/gemm_f32.hip)
# ----------------------------------------------------------------------------------------------------------------
def deep_fwd(shape, ldx):
    """cdm_convT2x2_fwd_x16 runs gemm_deep_kernel<DeepDenseA>"""
    N, H, W, Cin, Cout = shape
    return (N * H * W) % GBM == 0 and (4 * Cout) % GBN == 0 and Cin % 32 == 0 and ldx % 4 == 0


def deep_dgrad(shape, lddy):
    """cdm_convT2x2_dgrad_x16 runs gemm_deep_kernel<DeepConvT2x2GatherA>"""
    N, H, W, Cin, Cout = shape
    return (N * H * W) % GBM == 0 and Cin % GBN == 0 and Cout % 16 == 0 and (4 * Cout) % 32 == 0 and lddy % 4 == 0


def deep_grid(shape, dgrad=False):
    N, H, W, Cin, Cout = shape
    return (N * H * W // GBM, (Cin if dgrad else 4 * Cout) // GBN)


def tr_wgrad(shape, ldx, lddy):
    """cdm_convT2x2_wgrad_x16 runs convT2x2_wgrad_tr_kernel"""
    N, H, W, Cin, Cout = shape
    return Cin % 128 == 0 and Cout % 128 == 0 and W % 16 == 0 and ldx % 4 == 0 and lddy % 4 == 0


def tr_grid(shape, splits):
    N, H, W, Cin, Cout = shape
    return (Cin // GBM) * (4 * Cout // GBN) * effective_splits(N * H * W, splits)


def xcd_qr(nwg):
    """the XCD remap's (q, r): r != 0 is the remainder branch"""
    return nwg >> 3, nwg & 7


def reduce4(N, splits):
    """cdm_slab_reduce runs slab_reduce4_kernel"""
    return N % 4 == 0 and splits >= 8


def convT_fast_tiles(shape):
    """{(mw, nw): fast} per 64 x 64 wave tile of the ConvT forward: EpiConvT2x2's wave-uniform write-out (True) or its
    carry walk (False)"""
    N, H, W, Cin, Cout = shape
    M, NN = N * H * W, 4 * Cout
    ok = (W == 16 or W % 32 == 0) and (H * W) % 32 == 0
    return {(mw, nw): ok and mw + 64 <= M and nw + 64 <= NN
            for mw in range(0, -(-M // GBM) * GBM, 64) for nw in range(0, -(-NN // GBN) * GBN, 64) if mw < M and nw < NN}


def conv_inst(shape):
    """the instantiation of conv3x3_fwd_f32"""
    N, H, W, Cin, Cout = shape
    if Cin == 128 and Cout == 128:
        return "128-64" if H == 64 and W == 64 else "128"
    return "generic"


# ----------------------------------------------------------------------------------------------------------------
# wrong emulations of the ConvT scatter (tests/test_gemm_refs_cpu.py: the data must see them)
# ----------------------------------------------------------------------------------------------------------------
def convT_fwd_scatter(x, Wt, b, wrong):
    """the ConvT forward as GEMM + scatter, with one error:
    "seam": the input row taken as m / W without the reduction modulo H, on top of the image's own offset
    "row16": EpiConvT2x2's W == 16 offset of the second half of a 32-pixel block (4 W + 2 (d - 16) output pixels)
             applied at any W"""
    N, H, W, Ci = x.shape
    Co = Wt.shape[1]
    g = x.reshape(-1, Ci) @ convT_pack(Wt) + np.tile(b, 4)           # [m][ij Co + co]
    y = np.zeros((N * 2 * H * 2 * W, Co))
    m = np.arange(N * H * W)
    n, h, w = m // (H * W), (m // W) % H, m % W
    for ij in range(4):
        i, j = ij >> 1, ij & 1
        if wrong == "seam":
            pix = (n * 2 * H + 2 * (m // W) + i) * (2 * W) + 2 * w + j
        else:
            assert wrong == "row16"
            mb, d = m - m % 32, m % 32
            nb, hb, wb = mb // (H * W), (mb // W) % H, mb % W
            base = (nb * 2 * H + 2 * hb) * (2 * W) + 2 * wb
            pix = base + np.where(d < 16, 2 * d, 4 * W + 2 * (d - 16)) + i * 2 * W + j
        y[pix % y.shape[0]] = g[:, ij * Co:(ij + 1) * Co]
    return y.reshape(N, 2 * H, 2 * W, Co)


# ----------------------------------------------------------------------------------------------------------------
# case lists.  Shapes (N, H, W, Cin, Cout), H x W the input grid; `data` "exact" | "gauss"
# ----------------------------------------------------------------------------------------------------------------
# ConvT forward: (name, shape, x ld - Cin, x offset).  Comments: what the case reaches (asserted on the CPU)
FWD_CASES = [
    ("F0", (1, 4, 8, 16, 8), 4, 0),       # M = NN = 32: partial tiles both ways, carry walk, one K tile
    ("F1", (3, 2, 16, 36, 36), 4, 0),     # K tail 4, NN = 144, M = 96; W = 16, hw = 32: one wave tile fast, the rest walk
    ("F2", (3, 4, 32, 32, 32), 4, 0),     # deep, grid 3 x 1, nwg 3; H != W; fast path at W = 32
    ("F3", (1, 16, 16, 64, 96), 4, 0),    # deep, grid 2 x 3 = 6; W = 16 second-row offset inside full tiles
    ("F4", (11, 4, 32, 32, 32), 4, 0),    # deep, nwg 11 (q 1, r 3)
    ("F5", (2, 8, 8, 64, 32), 8, 4),      # deep at ldx = Cin + 8, offset 4; carry walk in full tiles (W = 8)
]
FWD_GAUSS = ("FG", (3, 2, 16, 36, 36), 4, 0)
# ConvT input gradient: K = 4 Cout, columns Cin
DGRAD_CASES = [
    ("D0", (1, 4, 8, 16, 8), 4, 0),       # generic, partial tiles
    ("D1", (3, 4, 32, 128, 16), 4, 0),    # deep, nwg 3, K = 64
    ("D2", (1, 8, 16, 256, 48), 4, 0),    # deep, grid 1 x 2; sub-pixel boundaries at k = 48, 96, 144 inside tile pairs
    ("D3", (2, 8, 8, 132, 20), 8, 4),     # Cout % 16 != 0: generic gather, a K tile straddles two sub-pixels; Cin tail
    ("D4", (11, 4, 32, 128, 16), 4, 0),   # deep, nwg 11
]
DGRAD_GAUSS = ("DG", (3, 4, 32, 128, 16), 4, 0)
DGRAD_FLAGS = (0, EPI_ACCUM, EPI_RELU | EPI_ACCUM)
# ConvT weight gradient: (name, shape, requested splits)
WGRAD_CASES = [
    ("W0", (2, 4, 8, 16, 8), (1, 3)),         # generic
    ("W1", (1, 2, 16, 128, 128), (1, 2)),     # tr, grid 4 / 8
    ("W2", (3, 3, 16, 128, 128), (4, 5)),     # 9 K tiles: per 3, 3 splits, grid 12 (r 4); per 2, 5 splits, last one tile
    ("W3", (1, 4, 32, 256, 128), (3,)),       # gx = 2, last split short
    ("W4", (2, 8, 8, 128, 128), (1, 3)),      # W % 16 != 0: generic at the tr channel counts
]
WGRAD_GAUSS = ("WG", (3, 3, 16, 128, 128), (4,))
# fp32 3x3 conv: (name, shape, kcs, flags, bias, stats)
CONV_CASES = [
    ("C0", (1, 4, 8, 8, 4), (0,), 0, True, True),                    # tiny partial tiles
    ("C1", (2, 6, 16, 16, 36), (0, 16), EPI_RELU, True, True),       # M = 192: two tiles, the second with 64 rows
    ("C2", (1, 8, 16, 128, 128), (0, 16), EPI_ACCUM, True, False),   # the <128, KC> instantiation
    ("C3", (2, 64, 64, 128, 128), (0, 16), 0, False, True),          # the hot <128, KC, 64> instantiation, 64 M tiles
    ("C4", (5, 8, 16, 16, 16), (0, 16), 0, False, True),             # 5 M tiles: remap remainder
    ("C5", (11, 8, 16, 128, 128), (0, 16), EPI_RELU, False, False),  # 11 tiles on <128, KC>
]
CONV_GAUSS = ("CG", (2, 6, 16, 16, 36), (16,), EPI_RELU, True, True)
CONV_WGRAD_SPLITS = (1, 7)
# dense GEMM (M, K, N): (name, shape, requested splits, [(bias_mod, flags)])
GEMM_CASES = [
    ("G0", (5, 36, 132), 1, [(132, 0), (4, 0), (4, EPI_RELU), (132, EPI_ACCUM), (0, EPI_RELU | EPI_ACCUM)]),
    ("G1", (130, 20, 4), 1, [(4, 0), (0, EPI_ACCUM)]),               # M tail of 2 rows past a tile; N = 4
    ("G2", (3, 272, 8), 16, []),                                     # 17 K tiles, per 2, 9 splits, last one tile
]
GEMM_GAUSS = ("GG", (5, 36, 132), 1, [(4, EPI_RELU | EPI_ACCUM)])
TN_CASES = [
    ("TN0", (8, 5, 12), 1),               # K smaller than a tile and not a multiple of 4 (the engine's K = batch)
    ("TN1", (132, 40, 260), 3),           # split K with M and N tails
]
TN_GAUSS = ("TNG", (132, 40, 260), 3)
# slab reduce
REDUCE_SHAPES = [(3, 8), (5, 36), (16, 132), (7, 6)]
REDUCE_SPLITS = [1, 3, 7, 8, 9, 16, 17, 24]


def reduce_perms(M, N):
    """[(name, s_m, s_hi, s_lo, csplit, buffer elements)]: the permutations the engine uses, N factored accordingly
    (N = taps x channels with the largest of 9 / 4 / 2 / 1 taps that divides it), and one with s_m > N"""
    out = [("identity", N, 0, 1, N, M * N), ("csplit0", N, 0, 1, 0, M * N), ("wide", N + 4, 0, 1, N, M * (N + 4))]
    for name, taps in (("oihw", 9), ("convT", 4), ("up0", 2)):
        if N % taps == 0:
            C = N // taps
            out.append((name, taps * C, 1, taps, C, M * N))
    return out


# ----------------------------------------------------------------------------------------------------------------
# case builders (cached; ops = 1: the reference's operands rounded to bf16, Gaussian nterm = 1 only)
# ----------------------------------------------------------------------------------------------------------------
@cached
def convT_case(shape, data, ops):
    """every operand of the three ConvT ops on one shape; the forward, input gradient (raw: the epilogue is applied
    by the test per flag set) and their sum|term|"""
    N, H, W, Ci, Co = shape
    rng = np.random.default_rng(_seed(*shape, data, 11))
    ex = data == "exact"
    x, Wt, b = operand(rng, (N, H, W, Ci), ex), operand(rng, (Ci, Co, 2, 2), ex, 0.1), operand(rng, Co, ex)
    dy, old = operand(rng, (N, 2 * H, 2 * W, Co), ex), operand(rng, (N, H, W, Ci), ex)
    xq, Wq, dyq = q16(x, ops), q16(Wt, ops), q16(dy, ops)
    return dict(x=x, Wt=Wt, b=b, dy=dy, old=old, xq=xq, Wq=Wq, dyq=dyq,
                y=convT_fwd(xq, Wq), y_mag=convT_fwd(np.abs(xq), np.abs(Wq)),
                dx=convT_dgrad(dyq, Wq), dx_mag=convT_dgrad(np.abs(dyq), np.abs(Wq)))


@cached
def conv_case(shape, data, ops):
    N, H, W, Ci, Co = shape
    rng = np.random.default_rng(_seed(*shape, data, 12))
    ex = data == "exact"
    x, Wt, b = operand(rng, (N, H, W, Ci), ex), operand(rng, (Co, Ci, 3, 3), ex, 0.05), operand(rng, Co, ex)
    gy, old = operand(rng, (N, H, W, Co), ex), operand(rng, (N, H, W, Co), ex)
    xq, Wq, gq = q16(x, ops), q16(Wt, ops), q16(gy, ops)
    return dict(x=x, Wt=Wt, b=b, gy=gy, old=old, xq=xq, Wq=Wq, gq=gq,
                y=conv3x3(xq, Wq), y_mag=conv3x3(np.abs(xq), np.abs(Wq)),
                dx=conv3x3_dgrad(gq, Wq), dx_mag=conv3x3_dgrad(np.abs(gq), np.abs(Wq)))


@cached
def gemm_case(shape, data, tn):
    """a [M][K] (tn: [K][M]), b [K][N], bias [N], old [M][N]"""
    M, K, N = shape
    rng = np.random.default_rng(_seed(*shape, data, 13 + tn))
    ex = data == "exact"
    return dict(a=operand(rng, (K, M) if tn else (M, K), ex), b=operand(rng, (K, N), ex), bias=operand(rng, N, ex),
                old=operand(rng, (M, N), ex))


@cached
def reduce_case(M, N, splits, data):
    rng = np.random.default_rng(_seed(M, N, splits, data, 14))
    ex = data == "exact"
    return dict(slab=operand(rng, (splits, M, N), ex), old=operand(rng, M * (N + 4), ex))


# torch fp64 references the functions above are held to (tests/test_gemm_refs_cpu.py)
def torch_convT(x, Wt, b, dy):
    """(y NHWC, dx NHWC, dW [Cin][Cout][2][2]) by conv_transpose2d and its autograd"""
    xt = _t(x).permute(0, 3, 1, 2).requires_grad_()
    wt = _t(Wt).requires_grad_()
    y = F.conv_transpose2d(xt, wt, _t(b), stride=2)
    y.backward(_t(dy).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy(), wt.grad.numpy()
