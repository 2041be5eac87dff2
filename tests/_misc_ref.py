"""fp64 CPU references, input generators and derived bounds for the small-op kernels of csrc/misc.hip (test
infrastructure shared by tests/test_gpu_misc_ops.py, which holds the kernels to them, and tests/test_misc_refs_cpu.py,
which holds these functions to torch's fp64 operators and autograd).

Every function takes and returns fp64 numpy arrays of values that are exactly representable in fp32.  Layouts are the
kernels': images [N, H, W], activations NHWC, the C_in = 1 weights w9[tap][c], the C_out = 1 weights w[c][tap], tap =
3 ky + kx with offset (ky - 1, kx - 1), zero padding.

Bounds (u = 2^-24; the vocabulary of tests/test_gpu_norm_ops.py):
  * a sequential fp32 chain of n multiply-adds: (n + 8) u sum|term|                                  chain_bound
  * an fp64 sum rounded once to fp32: 1 ulp(ref) + 2^-50 sum|term|                                    sum_bound
  * a chunked fp32 reducer, P = 256 / (C / 4) pixel lanes: n = ceil(pixels / P) + P (the lane's chain, then the fold
    over the lanes)                                                                                   lanes_n
  * fp32 GELU' = 1/2 + erf/2 + x pdf: 4 u (1/2 + |erf|/2 + |x| pdf)                                   gelu_grad
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SENT = 777.0
TAPS = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]


# ----------------------------------------------------------------------------------------------------------------
# helpers (as tests/test_gpu_norm_ops.py)
# ----------------------------------------------------------------------------------------------------------------
def dyad(rng, shape, step=2.0 ** -6, lim=4.0):
    k = int(round(lim / step))
    return rng.integers(-k, k + 1, size=shape).astype(np.float64) * step


def f32(a):
    """a rounded to fp32, as fp64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def gauss(rng, shape, scale=1.0):
    return f32(rng.standard_normal(shape) * scale)


def ulp(x):
    """spacing of fp32 at |x| (x: fp64 reference values)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def check(got, ref, bound, what):
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err - bound, -1.0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} beyond the bound; worst at {i}: got {got[i]!r}, "
                             f"ref {ref[i]!r}, err {err[i]:.3e} > {bound[i]:.3e}")


def exact(got, ref, what):
    check(got, ref, 0.0, what)


def widen(a, ld, off):
    """a [..., C] as a channel slice at offset `off` of a [..., ld] buffer filled with the sentinel"""
    buf = np.full(a.shape[:-1] + (ld,), SENT)
    buf[..., off:off + a.shape[-1]] = a
    return buf


def chain_bound(n, mag):
    return (n + 8) * U * np.asarray(mag, dtype=np.float64)


def sum_bound(ref, mag):
    return ulp(ref) + 2.0 ** -50 * np.asarray(mag, dtype=np.float64)


def lanes_n(C, pixels):
    lanes = 256 // (C // 4)
    return math.ceil(pixels / lanes) + lanes


def chunk_sums(a, csize):
    """a [N, HW, ...] -> [N, ceil(HW / csize), ...]: the sum over each chunk's own pixels"""
    return np.add.reduceat(a, np.arange(0, a.shape[1], csize), axis=1)


def grid_units(terms, step):
    """sum|term| in units of the dyadic grid `step`, the largest over the reduced axis 1: below 2^24, every partial
    sum, in any order, is an integer multiple of step below 2^24 steps, hence exact in fp32"""
    t = np.abs(terms) / step
    assert np.array_equal(t, np.round(t)), "terms are not on the grid"
    return float(t.sum(axis=1).max())


def sums_exact_in_fp32(terms):
    """the running sums over axis 1, in fp32 and in fp64, are equal"""
    a32 = np.cumsum(terms.astype(np.float32), axis=1, dtype=np.float32)
    a64 = np.cumsum(terms, axis=1, dtype=np.float64)
    return bool(np.array_equal(a32.astype(np.float64), a64))


# ----------------------------------------------------------------------------------------------------------------
# GELU (erf form, torch.nn.GELU())
# ----------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def gelu(x):
    """x Phi(x) with Phi = erfc(-x / sqrt 2) / 2: no cancellation in the negative tail"""
    return x * 0.5 * torch.special.erfc(-_t(x) / math.sqrt(2.0)).numpy()


def gelu_grad(x):
    """GELU'(x) = 1/2 + erf(x / sqrt 2) / 2 + x pdf(x), and the bound of its fp32 evaluation"""
    erf = torch.special.erf(_t(x) / math.sqrt(2.0)).numpy()
    cdf = 0.5 * torch.special.erfc(-_t(x) / math.sqrt(2.0)).numpy()
    pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf, 4 * U * (0.5 + 0.5 * np.abs(erf) + np.abs(x) * pdf)


# ----------------------------------------------------------------------------------------------------------------
# EmbedFC: out = W2 gelu(W1 x + b1) + b2, stage by stage
# ----------------------------------------------------------------------------------------------------------------
MLPS_A = [(5, 1, 16), (65, 6, 8), (130, 5, 100), (3, 8, 1024)]      # (rows, in_dim, E) of one launch
MLP_B = (5, 6, 64)


def embed_inputs(rng, rows, in_dim, E):
    """Gaussian weights (torch.nn.Linear-like scales), x uniform in [0, 1), a Gaussian output gradient"""
    return dict(x=f32(rng.random((rows, in_dim))), w1=gauss(rng, (E, in_dim), 1.0 / math.sqrt(in_dim)),
                b1=gauss(rng, E, 0.5), w2=gauss(rng, (E, E), 1.0 / math.sqrt(E)), b2=gauss(rng, E, 0.5),
                dout=gauss(rng, (rows, E)))


def embed_fwd(x, w1, b1, w2, b2):
    """pre, h, out in fp64 throughout, and sum|term| of out"""
    pre = x @ w1.T + b1
    h = gelu(pre)
    return pre, h, h @ w2.T + b2, np.abs(h) @ np.abs(w2).T + np.abs(b2)


def embed_dpre(dout, w2, pre):
    """dpre[b][i] = GELU'(pre[b][i]) sum_j dout[b][j] w2[j][i] from the stored fp32 pre; the bound: the fp32 chain
    over j times |GELU'|, the fp32 GELU' error times |sum|, and the final product's rounding"""
    s = dout @ w2
    gp, gp_err = gelu_grad(pre)
    ref = s * gp
    E = w2.shape[0]
    return ref, chain_bound(E, np.abs(dout) @ np.abs(w2)) * np.abs(gp) + gp_err * np.abs(s) + ulp(ref)


def embed_param_grads(dout, h, dpre, x):
    """{name: (ref, sum|term|)} of dw2[j][i], db2[j] (from dout, h) and dw1[i][k], db1[i] (from dpre, x)"""
    return dict(dw2=(dout.T @ h, np.abs(dout).T @ np.abs(h)), db2=(dout.sum(0), np.abs(dout).sum(0)),
                dw1=(dpre.T @ x, np.abs(dpre).T @ np.abs(x)), db1=(dpre.sum(0), np.abs(dpre).sum(0)))


def embed_input_grad(dpre_a, w1_a, dpre_b=None, w1_b=None):
    """dx[b][k] = sum_i dpre_a[b][i] w1_a[i][k] (+ the same of b): two fp32 chains and their sum's rounding"""
    ref = dpre_a @ w1_a
    bound = chain_bound(w1_a.shape[0], np.abs(dpre_a) @ np.abs(w1_a))
    if dpre_b is not None:
        ref = ref + dpre_b @ w1_b
        bound = bound + chain_bound(w1_b.shape[0], np.abs(dpre_b) @ np.abs(w1_b))
    return ref, bound + ulp(ref)


# ----------------------------------------------------------------------------------------------------------------
# MSE loss, its accumulating form, the forward perturbation
# ----------------------------------------------------------------------------------------------------------------
def mse_inputs(rng, n):
    """multiples of 2^-3 in [-1, 1]: d = pred - noise is a multiple of 2^-3 in [-2, 2], d^2 one of 2^-6 up to 4 = 256
    units, so a sum of n <= 65536 of them is at most 2^24 units: every partial sum is exact in fp32"""
    return dyad(rng, n, 2.0 ** -3, 1.0), dyad(rng, n, 2.0 ** -3, 1.0)


def mse_block_sums(v, n, nb):
    """[nb] sums of v over block b's elements i = (b * 256 + tid) + j * nb * 256 (the kernel's grid stride)"""
    blk = (np.arange(n) // 256) % nb
    return np.bincount(blk, weights=v, minlength=nb).astype(np.float64)


def mse_dbias_k(n, nb):
    """additions behind dbias = sum g: a thread's chain of ceil(n / (256 nb)) terms, 6 butterfly levels over the wave,
    the fold of the 4 waves (counted as 4), the finalize's fold of the nb block partials and its rounding to fp32
    (fp64: counted as nb all the same), and the vocabulary's + 8"""
    return math.ceil(n / (256 * nb)) + 6 + 4 + nb + 8


def mse_accum_k(HW):
    """sum d^2 of one sample: a thread's chain of ceil(HW / 256) terms, 6 butterfly levels, 3 adds over the waves, the
    + 8 of the vocabulary (which covers the roundings of d and d d in each term)"""
    return math.ceil(HW / 256) + 6 + 3 + 8


def mse_accum32(acc0, pred, noise, HW, mul, div):
    """the kernel's fp32 sequence after an exact sum d^2 (dyadic data): /HW, *mul, /div, += — four correctly rounded
    fp32 operations"""
    d = (pred - noise).reshape(-1, HW)
    s = (d * d).sum(axis=1)
    assert np.array_equal(s, f32(s))
    mse = s.astype(np.float32) / np.float32(HW)
    term = (mse * mul.astype(np.float32)) / div.astype(np.float32)
    return (acc0.astype(np.float32) + term).astype(np.float64)


def perturb32(x, nz, sab_t, omab_t):
    """sab[t] x + omab[t] nz with separate fp32 roundings ([N, HW] data, per-sample coefficients [N])"""
    a = sab_t.astype(np.float32)[:, None] * x.astype(np.float32)
    b = omab_t.astype(np.float32)[:, None] * nz.astype(np.float32)
    return (a + b).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------
# 3x3 convolutions with C_in = 1 or C_out = 1
# ----------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(2, 5, 7, 4), (1, 1, 1, 48), (3, 4, 1, 128), (1, 3, 300, 1024), (1, 16, 16, 128)]   # (N, H, W, C)
GRID = 2.0 ** -4     # conv data: multiples of 2^-4 in [-2, 2]; a product is a multiple of 2^-8 of at most 4 = 1024 units


def conv_dyad(rng, shape):
    return dyad(rng, shape, GRID, 2.0)


def shift(a, dh, dw):
    """b[n, h, w] = a[n, h + dh, w + dw], zero outside the image (a: [N, H, W, ...])"""
    H, W = a.shape[1:3]
    b = np.zeros_like(a)
    h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
    if h0 < h1 and w0 < w1:
        b[:, h0:h1, w0:w1] = a[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
    return b


def cin1_fwd(x, w9, b, relu):
    """y[p][c] = b[c] + sum_tap x[p + tap] w9[tap][c]; returns y and |b| + sum|x w|"""
    y = np.broadcast_to(b, x.shape + b.shape).copy(); mag = np.abs(y)
    for t, (dh, dw) in enumerate(TAPS):
        term = shift(x, dh, dw)[..., None] * w9[t]
        y += term; mag += np.abs(term)
    return (np.maximum(y, 0.0) if relu else y), mag


def cin1_wgrad_terms(dy, x):
    """[N, HW, 10, C]: rows 0..8 dy[p][c] x[p + tap], row 9 dy[p][c]"""
    N, H, W, C = dy.shape
    t = np.empty((N, H * W, 10, C))
    for r, (dh, dw) in enumerate(TAPS):
        t[:, :, r] = (dy * shift(x, dh, dw)[..., None]).reshape(N, H * W, C)
    t[:, :, 9] = dy.reshape(N, H * W, C)
    return t


def cout1_fwd(z, w, b, gs=None, gt=None):
    """out[p] = b + sum_{tap, c} z[p + tap][c] w[c][tap] (z = relu(z gs + gt) first, per (sample, channel)); returns
    out and |b| + sum|z w|"""
    if gs is not None:
        z = np.maximum(z * gs[:, None, None, :] + gt[:, None, None, :], 0.0)
    out = np.full(z.shape[:3], float(b)); mag = np.abs(out)
    for t, (dh, dw) in enumerate(TAPS):
        term = shift(z, dh, dw) * w[:, t]
        out += term.sum(-1); mag += np.abs(term).sum(-1)
    return out, mag


def cout1_dgrad(deps, w):
    """dz[p][c] = sum_tap deps[p - tap] w[c][tap]; returns dz and sum|deps w|"""
    dz = np.zeros(deps.shape + (w.shape[0],)); mag = np.zeros_like(dz)
    for t, (dh, dw) in enumerate(TAPS):
        term = shift(deps, -dh, -dw)[..., None] * w[:, t]
        dz += term; mag += np.abs(term)
    return dz, mag


def cout1_wgrad_chunk_terms(deps, z):
    """[N, HW, 9, C] indexed by the output pixel p: deps[p] z[p + tap][c]"""
    N, H, W, C = z.shape
    t = np.empty((N, H * W, 9, C))
    for r, (dh, dw) in enumerate(TAPS):
        t[:, :, r] = (deps[..., None] * shift(z, dh, dw)).reshape(N, H * W, C)
    return t


def cout1_wgrad_band_terms(deps, z, gs=None, gt=None):
    """[N, HW, 9, C] indexed by the input pixel q: z[q][c] deps[q - tap] (deps beyond the band comes from the halo)"""
    if gs is not None:
        z = np.maximum(z * gs[:, None, None, :] + gt[:, None, None, :], 0.0)
    N, H, W, C = z.shape
    t = np.empty((N, H * W, 9, C))
    for r, (dh, dw) in enumerate(TAPS):
        t[:, :, r] = (z * shift(deps, -dh, -dw)[..., None]).reshape(N, H * W, C)
    return t


def band_sums(terms, W, R):
    """[N, HW, 9, C] -> [N * H / R, 9, C]: the sum over each band of R whole rows"""
    N, HW = terms.shape[:2]
    return terms.reshape(N * (HW // (R * W)), R * W, *terms.shape[2:]).sum(axis=1)


# torch fp64 operators for the same layouts (the references the functions above are held to, and the GPU tests' own
# reference where the issue names torch's conv2d)
def torch_cin1(x, w9, b):
    """(conv2d module output NHWC as a torch tensor, leaf x, leaf weight [C, 1, 3, 3], leaf bias)"""
    C = w9.shape[1]
    xt = _t(x)[:, None].requires_grad_()
    wt = _t(w9.T.reshape(C, 1, 3, 3)).requires_grad_()
    bt = _t(b).requires_grad_()
    return torch.nn.functional.conv2d(xt, wt, bt, padding=1).permute(0, 2, 3, 1), xt, wt, bt


def torch_cout1(z, w, b):
    """(conv2d output [N, H, W], leaf z NCHW, leaf weight [1, C, 3, 3])"""
    C = w.shape[0]
    zt = _t(z.transpose(0, 3, 1, 2)).requires_grad_()
    wt = _t(w.reshape(1, C, 3, 3)).requires_grad_()
    return torch.nn.functional.conv2d(zt, wt, _t(np.array([float(b)])), padding=1)[:, 0], zt, wt
