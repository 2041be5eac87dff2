"""fp64 CPU references, exact-data generators and exactness predicates for the matrix-core 3x3 convolutions of
csrc/conv_kernels.h: the LDS-halo kernel (forward, BN-ReLU staging, BN-backward dgrad, the eval epilogues) and the
kernel-row weight gradient.  Shared by tests/test_gpu_halo_ops.py, which holds the kernels to them, and
tests/test_conv_refs_cpu.py, which holds these functions to torch's fp64 autograd and checks the exactness conditions.

Layouts: activations NHWC fp64 numpy arrays, weights OIHW.  check / exact / widen / SENT / chain_bound / sum_bound are
those of tests/_misc_ref.py.

The exact-data method.  Every operand is an integer multiple of a power of two ("unit") with few significant bits, so
that (1) it is representable in the 16-bit form the kernel stages it in (bf16 for nterm = 1, the scaled fp16 hi term
with a zero lo term for h3), (2) every product is a multiple of the product of the units and (3) the sum of |product|
over a whole dot product stays below 2^24 such units: every partial sum, in any order and grouping, is then an integer
below 2^24 units and exact in fp32.  The kernel's result must equal the fp64 reference bit for bit.  `budget` measures
(3) on the actual data, `fits_bf16` / `fits_h3` check (1); tests/test_conv_refs_cpu.py asserts them for every case.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from _misc_ref import SENT, U, chain_bound, check, dyad, exact, f32, gauss, sum_bound, ulp, widen  # noqa: F401

EPI_RELU, EPI_ACCUM = 1, 2
NT_H3 = 4
G3 = 2.0 ** -3
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def bf16(a):
    """a (values representable in fp32) rounded to bf16, round to nearest even, as fp64: the kernels' (__bf16)
    conversion, the same torch conversion tests/_bf16emu.py rounds its operands with"""
    return _t(a).float().to(torch.bfloat16).double().numpy()


# ----------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------
def d3(rng, shape, lim=1.0):
    """integer multiples of 2^-3 in [-lim, lim]"""
    return dyad(rng, shape, G3, lim)


def pick(rng, shape, values):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), size=shape)]


def both_signs(rng, a):
    """a with its first two entries along the last axis forced to +max|a| / -max|a| (both signs in every case)"""
    a = np.array(a, dtype=np.float64)
    m = max(float(np.abs(a).max()), G3)
    a[..., 0], a[..., 1] = m, -m
    return a


def bn_relu_coeffs(rng, C, exact_data=True, coarse=False):
    """pre_s in {+-1/2, +-1, +-2}, pre_t a multiple of 2^-3 in [-1, 1] with both signs (Gaussian when not exact);
    coarse (the weight gradient's long sums): pre_s in {+-1, +-2}, so that z stays a multiple of 2^-3"""
    if not exact_data:
        return f32(gauss(rng, C) * 0.5 + 1.0), gauss(rng, C, 0.3)
    s = pick(rng, C, [1.0, -1.0, 2.0, -2.0] if coarse else [0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    return s, both_signs(rng, d3(rng, C))


def bn_bwd_coeffs(rng, C, kind="exact"):
    """(s, t, mean, invstd, A, B, Cc) per channel.
    exact: A in +-{1, 2}, Cc in +-{1/2, 1}, invstd in {1, 2} (invstd = 1 / sqrt(var + eps) is positive by definition,
      and cdm_bn_bwd_amax_bound takes it so), B and mean nonzero multiples of 2^-3 in [-1, 1]: with g, y multiples of
      2^-3 in [-1, 1], dy = A g' + B + Cc (y - mean) invstd is a multiple of 2^-4 below 2 + 1 + 4 < 8: 7 significant
      bits, so its bf16 rounding is the identity; B != 0 and Cc mean invstd != 0 on every channel.
    fine: the same with invstd in {1/8, 1/16}: dy is a multiple of 2^-8 of magnitude up to 3.5, so the bf16 rounding of
      the one-term staging is not the identity (still exact in fp32 and in the fp16 hi term).
    coarse (the weight gradient's sums over up to 12,288 pixels): as exact with Cc in +-1: dy is a multiple of 2^-3.
    gauss: Gaussian coefficients, invstd > 0."""
    if kind == "gauss":
        co = [gauss(rng, C) for _ in range(7)]
        co[0] = co[0] * 0.5 + 1.0
        co[3] = np.abs(co[3]) + 0.1
        return tuple(f32(c) for c in co)
    s, t = bn_relu_coeffs(rng, C)
    nz = np.array([k * G3 for k in range(-8, 9) if k != 0])
    mean, B = pick(rng, C, nz), pick(rng, C, nz)
    invstd = pick(rng, C, [0.125, 0.0625] if kind == "fine" else [1.0, 2.0])
    A = pick(rng, C, [1.0, -1.0, 2.0, -2.0])
    Cc = pick(rng, C, [1.0, -1.0] if kind == "coarse" else [0.5, -0.5, 1.0, -1.0])
    return s, t, mean, invstd, A, B, Cc


# ----------------------------------------------------------------------------------------------------------------
# the convolution, its input gradient and its weight gradient (torch fp64)
# ----------------------------------------------------------------------------------------------------------------
def conv3x3(x, W, bias=None):
    """y[n, h, w, o] = bias[o] + sum_{i, ky, kx} x[n, h + ky - 1, w + kx - 1, i] W[o, i, ky, kx], zero padding"""
    return _nhwc(F.conv2d(_nchw(x), _t(W), None if bias is None else _t(bias), padding=1))


def conv3x3_mag(x, W, bias=None):
    """sum |term| of conv3x3"""
    return conv3x3(np.abs(x), np.abs(W), None if bias is None else np.abs(bias))


def conv3x3_dgrad(gy, W):
    """dx[n, h, w, i] = sum_{o, ky, kx} gy[n, h - ky + 1, w - kx + 1, o] W[o, i, ky, kx]"""
    return _nhwc(F.conv_transpose2d(_nchw(gy), _t(W), padding=1))


def conv3x3_wgrad(gy, x):
    """dW[o, i, ky, kx] = sum_{n, h, w} gy[n, h, w, o] x[n, h + ky - 1, w + kx - 1, i]"""
    Cout, Cin = gy.shape[-1], x.shape[-1]
    return torch.nn.grad.conv2d_weight(_nchw(x), (Cout, Cin, 3, 3), _nchw(gy), padding=1).numpy()


# ----------------------------------------------------------------------------------------------------------------
# staging transforms
# ----------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on fp32 values held as fp64, correctly rounded.  The product is exact in fp64 (48 bits); the fp64 sum is
    taken in round-to-odd (TwoSum gives its exact error; an inexact sum whose last bit is even moves to the odd
    neighbour on the error's side), which carries enough to make the final rounding to fp32 the rounding of the exact
    a b + c: 53 >= 24 + 2 bits, no double rounding."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    move = (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
    return f32(np.where(move, odd, s))


def bn_relu_stage(x, s, t, to_bf16=False, f32ops=False):
    """z = relu(x s + t) per channel (last axis); f32ops: the kernel's one fmaf in fp32; to_bf16: then rounded to bf16
    (the one-term staging).  On exact data f32ops changes nothing."""
    z = np.maximum(fma32(x, s, t) if f32ops else x * s + t, 0.0)
    return bf16(z) if to_bf16 else z


def bn_bwd_stage(g, y, s, t, mean, invstd, A, B, Cc, to_bf16=False, f32ops=False):
    """dy = A (y s + t > 0 ? g : 0) + B + Cc (y - mean) invstd (include/cdm_hip.h, cdm_conv3x3_dgrad_x16_bnbwd_dy);
    f32ops: the kernel's fp32 sequence zp = fmaf(y, s, t), xh = (y - mean) * invstd, fmaf(Cc, xh, fmaf(A, g', B))."""
    if f32ops:
        zp = fma32(y, s, t)
        xh = f32(f32(y - mean) * invstd)
        dy = fma32(Cc, xh, fma32(A, np.where(zp > 0, g, 0.0), B))
    else:
        dy = A * np.where(y * s + t > 0, g, 0.0) + B + Cc * (y - mean) * invstd
    return bf16(dy) if to_bf16 else dy


# ----------------------------------------------------------------------------------------------------------------
# epilogues
# ----------------------------------------------------------------------------------------------------------------
def epilogue(v, flags, old=None, bias=None, to_bf16=False):
    """bias, then += old (EPI_ACCUM), then relu (EPI_RELU), then the store rounding: the kernel's order"""
    if bias is not None:
        v = v + bias
    if flags & EPI_ACCUM:
        v = v + old
    if flags & EPI_RELU:
        v = np.maximum(v, 0.0)
    return bf16(f32(v)) if to_bf16 else v


def tile_stats(y):
    """y [..., C] -> (sums, sums of squares), each [ceil(pixels / 128), C]; a partial last tile sums the rows that exist"""
    y = y.reshape(-1, y.shape[-1])
    if y.shape[0] % 128:
        y = np.concatenate([y, np.zeros((-y.shape[0] % 128, y.shape[1]))])
    t = y.reshape(-1, 128, y.shape[-1])
    return t.sum(1), (t * t).sum(1)


def fkey(f):
    """the ordered-int key of an fp32 value (as tests/test_gpu_norm_ops.py)"""
    i = np.asarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF).astype(np.int32)


def ymm_keys(y):
    """[2, C]: the keys of the per-channel max and min of y"""
    y2 = y.reshape(-1, y.shape[-1])
    return np.stack([fkey(y2.max(0)), fkey(y2.min(0))])


def eval_fused(kind, v, sc_x=None, sc_w=None, sc_b=None, split=0, fa=None, fb=None):
    """the eval epilogues on v = relu(conv + bias) [N, H, W, C] (include/cdm_hip.h, cdm_conv3x3_fwd_x16_fused):
    kind 1: sc_w[s][c] sc_x[n, h, w] + sc_b[s][c] + v with s = (image >= split); sc_w, sc_b [2, C]
    kind 2: fa[n][c] v + fb[n][c]; fa, fb [N, C] (a shared row is passed broadcast)
    kind 3: the 2 x 2 max, [N, H/2, W/2, C]"""
    N, H, W, C = v.shape
    if kind == 1:
        sel = (np.arange(N) >= split).astype(int)
        return sc_w[sel][:, None, None, :] * sc_x[..., None] + sc_b[sel][:, None, None, :] + v
    if kind == 2:
        return np.broadcast_to(fa, (N, C))[:, None, None, :] * v + np.broadcast_to(fb, (N, C))[:, None, None, :]
    assert kind == 3
    return v.reshape(N, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


# ----------------------------------------------------------------------------------------------------------------
# exactness predicates
# ----------------------------------------------------------------------------------------------------------------
def unit(a):
    """the largest power of two of which every element of a is an integer multiple (1 for an all-zero array)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[a > 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)                                   # a = m 2^e, m in [0.5, 1): m 2^53 is an integer
    k = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2((k & -k).astype(np.float64)) + e - 53  # exponent of the lowest set bit
    return 2.0 ** float(low.min())


def budget(mag, *operands):
    """max sum|term| in units of the finest grid of the result: the product of the first two operands' units, and the
    units of any further addend (bias, old value).  Below 2^24: every partial sum is exact in fp32."""
    u = unit(operands[0]) * unit(operands[1])
    for o in operands[2:]:
        if o is not None:
            u = min(u, unit(o))
    return float(np.max(mag)) / u


def fits_bf16(a):
    return bool(np.array_equal(bf16(a), np.asarray(a, dtype=np.float64)))


def h3_scale(amax):
    """the h3 operand scale 2^(14 - e), amax = f 2^e with f in [0.5, 1)"""
    return 2.0 ** (14 - math.frexp(float(amax))[1])


def fits_h3(a, amax):
    """a 2^(14 - e) is exact in fp16 (the hi term; the lo term is then zero)"""
    v = np.asarray(a, dtype=np.float64) * h3_scale(amax)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(v.astype(np.float16).astype(np.float64), v))


def fits16(a, nterm, amax=None):
    return fits_bf16(a) if nterm == 1 else fits_h3(a, np.abs(a).max() if amax is None else amax)


def fp32_exact(a):
    return bool(np.array_equal(f32(a), np.asarray(a, dtype=np.float64)))


# ----------------------------------------------------------------------------------------------------------------
# the weight gradient's host-side dispatch, restated: which K step a case really gets.  tests/test_conv_refs_cpu.py
# holds the KS each case of the GPU file declares to this; the GPU file holds the split counts to the library's.
# ----------------------------------------------------------------------------------------------------------------
WGRAD_BLOCKS = 768   # engine.WGRAD_BLOCKS


def effective_splits(K, splits, BK=16):
    """effective_splits of csrc/conv_kernels.h (cdm_gemm_splits at BK = 16): the number of non-empty splits when K
    pixels in BK-pixel steps are dealt to `splits` splits of equal step count"""
    kt = (K + BK - 1) // BK
    splits = max(1, splits)
    if splits > kt:
        splits = kt if kt > 0 else 1
    per = (kt + splits - 1) // splits
    return (kt + per - 1) // per if kt > 0 else 1


def engine_wgrad_splits(K, Cout, Cin):
    """engine.wgrad_splits(K, Cout, 9 Cin) for the kernel-row shapes (Cin, Cout % 128 == 0): 768 blocks over
    3 (Cout / 128) (Cin / 128) blocks per split"""
    per = 3 * (Cout // 128) * (Cin // 128)
    return effective_splits(K, max(1, min(512, round(WGRAD_BLOCKS / per))))


def wgrad_ks(N, W, splits, nterm, dt):
    """the KS (K step = 16 KS pixels) cdm_conv3x3_wgrad_x16_ex dispatches (csrc/conv_wgrad.hip): a step size is taken
    only if the split count at that step size equals the one at 16 pixels; 4 (64 pixels) for h3 and for bf16 operands
    (dt != 0) at W % 64 == 0, else 2 at W % 32 == 0, else 1; 0: rejected"""
    K = N * W * W
    sp = effective_splits(K, splits)
    ks2 = W % 32 == 0 and effective_splits(K, splits, 32) == sp
    ks4 = W % 64 == 0 and effective_splits(K, splits, 64) == sp
    if not ks2 and effective_splits(K, splits, 16) != sp:
        return 0
    if ks4 and (dt != 0 or nterm == NT_H3):
        return 4
    return 2 if ks2 else 1


# ----------------------------------------------------------------------------------------------------------------
# case builders (CPU only; shared by the GPU tests and the CPU predicate test, cached so that the two arithmetics of a
# case share one reference).  Each returns a dict of inputs, the reference `ref`, sum|term| `mag`, and `mode`:
#   "exact"  bit-equal                               (exact data)
#   "h3"     2e-5 max|ref| + 1e-5                    (Gaussian data, h3: test_gpu_kernels._close)
#   "chain"  chain_bound(n, mag) per element         (Gaussian data or a non-identity bf16 staging, nterm = 1; the
#                                                     reference is the fp64 result of the operands rounded to bf16)
# ----------------------------------------------------------------------------------------------------------------
_CACHE = {}


def cached(fn):
    def wrap(*key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            if len(_CACHE) >= 3:
                _CACHE.pop(next(iter(_CACHE)))
            _CACHE[k] = fn(*key)
        return _CACHE[k]
    wrap.__name__ = fn.__name__
    return wrap


def _seed(*key):
    """a seed that depends on the case alone (not on the process: no hash())"""
    return sum((i + 1) * 7919 * (len(k) + ord(k[0]) if isinstance(k, str) else int(k)) for i, k in enumerate(key)) % 2 ** 31


def _mode(data, nterm):
    return "exact" if data == "exact" else ("h3" if nterm == NT_H3 else "chain")


def _ops(data, nterm):
    """operand arithmetic of the reference: 1 = operands rounded to bf16 (only Gaussian data needs it: exact data is
    its own bf16 image), 0 = as given"""
    return 1 if (data != "exact" and nterm == 1) else 0


def _q(a, ops):
    return bf16(a) if ops else a


@cached
def fwd_case(W, N, Cin, Cout, flags, bias, data, ops):
    """(a) plain forward: y = epilogue(conv(x) [+ bias] [+ old])"""
    rng = np.random.default_rng(_seed(W, N, Cin, Cout, flags, bias, data))
    sh = (N, W, W, Cin)
    if data == "exact":
        x, Wt, b = d3(rng, sh), d3(rng, (Cout, Cin, 3, 3)), both_signs(rng, d3(rng, Cout))
        old = d3(rng, (N, W, W, Cout), 4.0)
    else:
        x, Wt, b = gauss(rng, sh), gauss(rng, (Cout, Cin, 3, 3), 0.05), gauss(rng, Cout)
        old = gauss(rng, (N, W, W, Cout))
    b = b if bias else None
    old = old if flags & EPI_ACCUM else None
    xq, Wq = _q(x, ops), _q(Wt, ops)
    v, mag = conv3x3(xq, Wq), conv3x3_mag(xq, Wq, b)
    if old is not None:
        mag = mag + np.abs(old)
    return dict(x=x, Wt=Wt, b=b, old=old, xq=xq, Wq=Wq, ref=epilogue(v, flags, old, b), mag=mag)


@cached
def pre_case(W, N, Cin, Cout, dt, data, ops):
    """(b) forward on z = relu(x pre_s + pre_t) staged, bias, statistics, max / min keys; dt & 2: y stored as bf16"""
    rng = np.random.default_rng(_seed(W, N, Cin, Cout, dt, data, 2))
    ex = data == "exact"
    x = d3(rng, (N, W, W, Cin)) if ex else gauss(rng, (N, W, W, Cin))
    Wt = d3(rng, (Cout, Cin, 3, 3)) if ex else gauss(rng, (Cout, Cin, 3, 3), 0.05)
    b = both_signs(rng, d3(rng, Cout)) if ex else gauss(rng, Cout)
    s, t = bn_relu_coeffs(rng, Cin, ex)
    z = bn_relu_stage(x, s, t, to_bf16=bool(ops), f32ops=not ex)
    Wq = _q(Wt, ops)
    v, mag = conv3x3(z, Wq), conv3x3_mag(z, Wq, b)
    return dict(x=x, Wt=Wt, b=b, s=s, t=t, z=z, Wq=Wq, ref=epilogue(v, 0, None, b, to_bf16=bool(dt & 2)), mag=mag,
                z_plain=bn_relu_stage(x, s, t), z_f32=bn_relu_stage(x, s, t, f32ops=True))


@cached
def dgrad_case(W, N, C, Cout, flags, dt, kind, ops):
    """(c) out = epilogue(dgrad of dy = bn_bwd_stage(g, y, ...)); weights OIHW [C][Cout][3][3] of the forward conv
    Cout -> C whose input gradient this is; ops: dy rounded to bf16 (the one-term staging)"""
    rng = np.random.default_rng(_seed(W, N, C, Cout, flags, dt, kind, 3))
    ex = kind != "gauss"
    sh = (N, W, W, C)
    g, y = (d3(rng, sh), d3(rng, sh)) if ex else (gauss(rng, sh), f32(gauss(rng, sh, 2.0) + 0.25))
    Wt = d3(rng, (C, Cout, 3, 3)) if ex else gauss(rng, (C, Cout, 3, 3), 0.05)
    old = (d3(rng, (N, W, W, Cout), 4.0) if ex else gauss(rng, (N, W, W, Cout))) if flags & EPI_ACCUM else None
    co = bn_bwd_coeffs(rng, C, kind)
    dy32 = bn_bwd_stage(g, y, *co, f32ops=True)                   # what dy_out holds (then g's element type)
    dy = bf16(dy32) if ops else dy32
    Wq = _q(Wt, ops)
    v, mag = conv3x3_dgrad(dy, Wq), conv3x3_dgrad(np.abs(dy), np.abs(Wq))
    if old is not None:
        mag = mag + np.abs(old)
    return dict(g=g, y=y, Wt=Wt, Wq=Wq, old=old, co=co, dy=dy, dy32=dy32, dy_plain=bn_bwd_stage(g, y, *co),
                ref=epilogue(v, flags, old, None, to_bf16=bool(dt & 2)), mag=mag)


@cached
def fused_case(kind, W, Cin, Cout, var, data, ops):
    """(d) eval epilogues on v = relu(conv + bias), N = 3.  kind 1: var = split; kind 2: var = 0 shared FiLM rows,
    1 per-image rows; kind 3: a block of zero input (ties inside pooling windows) and strongly negative biases
    (windows whose maximum is 0 after the relu)"""
    N = 3
    rng = np.random.default_rng(_seed(kind, W, Cin, Cout, var, data, 4))
    ex = data == "exact"
    x = d3(rng, (N, W, W, Cin)) if ex else gauss(rng, (N, W, W, Cin))
    Wt = d3(rng, (Cout, Cin, 3, 3)) if ex else gauss(rng, (Cout, Cin, 3, 3), 0.05)
    b = both_signs(rng, d3(rng, Cout)) if ex else gauss(rng, Cout)
    r = lambda *sh: d3(rng, sh) if ex else gauss(rng, sh)    # noqa: E731
    d = dict(sc_x=r(N, W, W), sc_w=r(2, Cout), sc_b=r(2, Cout), fa=r(N if var else 1, Cout), fb=r(N if var else 1, Cout))
    if kind == 3:
        x[:, 2:12, 3:13] = 0.0
        b[5::16] = -512.0
    xq, Wq = _q(x, ops), _q(Wt, ops)
    v = np.maximum(conv3x3(xq, Wq, b), 0.0)
    mag = conv3x3_mag(xq, Wq, b)
    ref = eval_fused(kind, v, d["sc_x"], d["sc_w"], d["sc_b"], var, d["fa"], d["fb"])
    if kind == 2:
        mag = eval_fused(2, mag, fa=np.abs(d["fa"]), fb=np.abs(d["fb"]))
    elif kind == 3:
        mag = mag.reshape(N, W // 2, 2, W // 2, 2, Cout).max(axis=(2, 4))
    else:
        mag = eval_fused(1, mag, np.abs(d["sc_x"]), np.abs(d["sc_w"]), np.abs(d["sc_b"]), var)
    return dict(x=x, Wt=Wt, b=b, xq=xq, Wq=Wq, v=v, ref=ref, mag=mag, **d)


@cached
def wgrad_case(Cin, Cout, W, N, bn, px, kind, ops):
    """(e) dW = weight gradient of dY (plain g, or bn_bwd_stage(g, y, ...) when bn) and X (plain x, or
    relu(x x_s + x_t) when px); ops: both staged operands rounded to bf16"""
    rng = np.random.default_rng(_seed(Cin, Cout, W, N, bn, px, kind, 5))
    ex = kind != "gauss"
    sg, sx = (N, W, W, Cout), (N, W, W, Cin)
    g, y = (d3(rng, sg), d3(rng, sg)) if ex else (gauss(rng, sg), f32(gauss(rng, sg, 2.0) + 0.25))
    x = d3(rng, sx) if ex else gauss(rng, sx)
    co = bn_bwd_coeffs(rng, Cout, "coarse" if kind == "exact" else kind)
    xs, xt = bn_relu_coeffs(rng, Cin, ex, coarse=True)
    dy = bn_bwd_stage(g, y, *co, f32ops=True) if bn else g
    X = bn_relu_stage(x, xs, xt, f32ops=True) if px else x
    dyq, Xq = _q(dy, ops), _q(X, ops)
    return dict(g=g, y=y, x=x, co=co, xs=xs, xt=xt, dy=dyq, X=Xq, dy_plain=bn_bwd_stage(g, y, *co) if bn else g,
                X_plain=bn_relu_stage(x, xs, xt) if px else x, ref=conv3x3_wgrad(dyq, Xq),
                mag=conv3x3_wgrad(np.abs(dyq), np.abs(Xq)))
