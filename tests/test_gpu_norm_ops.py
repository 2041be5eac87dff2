"""Direct tests of the normalisation / reduction kernels (csrc/norm.hip, and cdm_slab_sum_all / cdm_avgpool_gelu_* of
csrc/misc.hip) against plain fp64 numpy / torch references on the CPU (GPU box only).

Inputs.  "Dyadic" inputs make fp32 arithmetic exact: y, g multiples of 2^-6 in [-4, 4]; s, t, A, B, Cc, FiLM and
shortcut coefficients multiples of 2^-4 in [-2, 2]; mean = 0 and invstd a power of two.  Then fmaf(y, s, t) is exact,
so the ReLU gate, the pool argmax and its ties equal the fp64 reference element for element, elementwise results are
compared bit for bit, and fp64 folds of such values are exact in any order.  The end-to-end chains use Gaussian data
(fixed seeds, chosen on the CPU so that no pre-activation lies within 1e-6 of the gate; asserted).

Tolerances (derived, u = 2^-24):
  * fp32 partial sum of n_add sequential additions of fp32-computed terms: (n_add + 8) u sum|term|.  Chunked reducers:
    n_add = T ceil(csize / P) + P with P = 256 / (C / 4) pixel lanes (the per-lane chain, then the fold over lanes) and
    T the terms a lane adds per pixel: 1, or 4 in the pooled mode (the four elements of a 2x2 window).
  * fp64 fold rounded once to fp32: 1 ulp of the fp64 result; with one further fp32 multiply-add: 2 ulp of the
    largest term.  cdm_slab_colsum (fp64 out): 2^-50 sum|v|.
  * elementwise apply: 4 u (sum of the magnitudes of its terms); bit-equal on dyadic inputs.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = float(np.float32(1e-5))     # the kernels take eps as a float
SENT = 777.0


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cdm_amd
    return cdm_amd.lib()


def _err():
    import cdm_amd
    return cdm_amd._lib.HipError


def _s():
    return torch.cuda.current_stream().cuda_stream if DEV == "cuda" else None


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype).to(DEV)


def Z(*shape, fill=SENT, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def Hh(t):
    _sync()
    return t.detach().cpu().numpy().astype(np.float64)


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t, off=0):
    """device address of t (+ off elements); t stays alive until the test ends (launches are asynchronous, and a
    temporary's memory would be handed to the next allocation)"""
    if t is None:
        return None
    _KEEP.append(t)
    return t.data_ptr() + off * t.element_size()


def dyad(rng, shape, step=2.0 ** -6, lim=4.0):
    k = int(round(lim / step))
    return rng.integers(-k, k + 1, size=shape).astype(np.float64) * step


def coef(rng, shape):
    return dyad(rng, shape, 2.0 ** -4, 2.0)


def pow2(rng, shape):
    return 2.0 ** rng.integers(-1, 2, size=shape).astype(np.float64)


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


def win(a):
    """[N, H, W, C] -> [N, H/2, W/2, 4, C], window element e = 2 dh + dw"""
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def unwin(a):
    N, Ho, Wo, _, C = a.shape
    return a.reshape(N, Ho, Wo, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)


def bc(v):
    """per-(sample | all, channel) coefficient [Ns, C] broadcast over an NHWC tensor"""
    return v[:, None, None, :]


def pieces(y, s, t, mean, invstd, cpg):
    zp = y * bc(s) + bc(t)
    xh = (y - bc(np.repeat(mean, cpg, axis=1))) * bc(np.repeat(invstd, cpg, axis=1))
    return zp, xh


def bwd_ref(mode, g, y, s, t, mean, invstd, cpg, fa):
    """gpre, xh (full grid) and the five backward terms with their magnitudes, per pixel of the reduced grid
    [N, HWp, C] (mode 1: summed over the 2x2 window); first index wins a pool tie (torch's MaxPool2d)."""
    N, H, W, C = y.shape
    zp, xh = pieces(y, s, t, mean, invstd, cpg)
    zero = np.zeros_like(y)
    if mode == 1:
        zw = win(np.maximum(zp, 0.0))
        arg = np.argmax(zw, axis=3)                       # first maximum
        hit = (np.arange(4)[None, None, None, :, None] == arg[:, :, :, None, :]) & (win(zp) > 0)
        gpre = unwin(np.where(hit, g[:, :, :, None, :], 0.0))
        red = lambda a: win(a).sum(axis=3).reshape(N, -1, C)   # noqa: E731
        terms = [red(gpre), red(gpre * xh), None, None, red(xh)]
        mags = [red(np.abs(gpre)), red(np.abs(gpre * xh)), None, None, red(np.abs(xh))]
        return gpre, xh, zp, terms, mags
    gz = g * bc(fa) if mode == 2 else g
    gpre = np.where(zp > 0, gz, zero)
    fl = lambda a: a.reshape(N, H * W, C)   # noqa: E731
    terms = [fl(gpre), fl(gpre * xh), None, None, fl(xh)]
    if mode == 2:
        terms[2] = fl(g * np.maximum(zp, 0.0)); terms[3] = fl(g)
    mags = [None if a is None else np.abs(a) for a in terms]
    return gpre, xh, zp, terms, mags


def chunk_sums(a, csize):
    return np.add.reduceat(a, np.arange(0, a.shape[1], csize), axis=1)


def n_add(C, csize, per_pixel=1):
    lanes = 256 // (C // 4)
    return per_pixel * math.ceil(csize / lanes) + lanes


def fkey(f):
    i = np.asarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF).astype(np.int32)


def fkey_inv(k):
    k = np.asarray(k, dtype=np.int32)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF).astype(np.int32).view(np.float32).astype(np.float64)


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------
# chunked reducers
# ----------------------------------------------------------------------------------------------------------------
def _norm_params(rng, N, C, gn):
    if gn:
        G = 8
        return dict(s=coef(rng, (N, C)), t=coef(rng, (N, C)), mean=np.zeros((N, G)), invstd=pow2(rng, (N, G)), sn=C,
                    mn=G, cpg=C // G)
    return dict(s=coef(rng, (1, C)), t=coef(rng, (1, C)), mean=np.zeros((1, C)), invstd=pow2(rng, (1, C)), sn=0, mn=0,
                cpg=1)


def _run_bwd_reduce(L, mode, g, y, np_, fa, film_an, csize, wide):
    N, H, W, C = y.shape
    Hg, Wg = (H // 2, W // 2) if mode == 1 else (H, W)
    ld, off = (C + 8, 4) if wide else (C, 0)
    yd = T(widen(y, ld, off)); gd = T(widen(g, ld, off))
    nch = -(-(Hg * Wg) // csize)
    slab = Z(N, nch, 5, C)
    fad = T(fa) if fa is not None else None
    L.cdm_norm_bwd_reduce(mode, P(gd, off), ld, P(yd, off), ld, N, H, W, C, P(T(np_["s"])), P(T(np_["t"])), np_["sn"],
                          P(T(np_["mean"])), P(T(np_["invstd"])), np_["mn"], np_["cpg"], P(fad), film_an, csize,
                          P(slab), _s())
    return Hh(slab)


def _check_bwd_slab(slab, terms, mags, C, csize, per_pixel, what):
    k = n_add(C, csize, per_pixel) + 8
    for r in range(5):
        if terms[r] is None:
            exact(slab[:, :, r], np.zeros_like(slab[:, :, r]), f"{what} row {r} (zero)")
        else:
            check(slab[:, :, r], chunk_sums(terms[r], csize), k * U * chunk_sums(mags[r], csize), f"{what} row {r}")


PIX = [(1, 5, 128, False), (8, 16, 128, False), (10, 20, 128, True), (10, 20, 200, False)]


@pytest.mark.parametrize("H,W,csize,wide", PIX)
@pytest.mark.parametrize("C", [4, 8, 48, 256, 1024])
def test_reduce_stats_sum_bwd(L, C, H, W, csize, wide):
    rng = np.random.default_rng(C * 1000 + H * W + csize)
    N, HW = 3, H * W
    y = dyad(rng, (N, H, W, C)); g = dyad(rng, (N, H, W, C))
    ld, off = (C + 8, 4) if wide else (C, 0)
    yd = T(widen(y, ld, off))
    nch = -(-HW // csize)
    k = n_add(C, csize) + 8
    yf = y.reshape(N, HW, C)
    slab = Z(N, nch, 2, C)
    L.cdm_reduce_stats(P(yd, off), ld, N, HW, C, csize, P(slab), _s())
    got = Hh(slab)
    check(got[:, :, 0], chunk_sums(yf, csize), k * U * chunk_sums(np.abs(yf), csize), "reduce_stats sum")
    check(got[:, :, 1], chunk_sums(yf * yf, csize), k * U * chunk_sums(yf * yf, csize), "reduce_stats sumsq")
    slab1 = Z(N, nch, 1, C)
    L.cdm_reduce_sum(P(yd, off), ld, N, HW, C, csize, P(slab1), _s())
    check(Hh(slab1)[:, :, 0], chunk_sums(yf, csize), k * U * chunk_sums(np.abs(yf), csize), "reduce_sum")
    for gn in ([False, True] if C % 8 == 0 else [False]):
        np_ = _norm_params(rng, N, C, gn)
        fa = coef(rng, (N, C))
        for mode in (0, 2):
            got = _run_bwd_reduce(L, mode, g, y, np_, fa if mode == 2 else None, C, csize, wide)
            _, _, _, terms, mags = bwd_ref(mode, g, y, np_["s"], np_["t"], np_["mean"], np_["invstd"], np_["cpg"], fa)
            _check_bwd_slab(got, terms, mags, C, csize, 1, f"bwd_reduce mode {mode} gn={gn}")


def tie_y(rng, shape):
    """y on a coarse grid (multiples of 1/2, still dyadic) so that many 2x2 windows tie"""
    return dyad(rng, shape, 0.5, 4.0)


def tie_share(y, s, t):
    zw = win(np.maximum(y * bc(s) + bc(t), 0.0))
    mx = zw.max(axis=3, keepdims=True)
    return float((((zw == mx).sum(axis=3) >= 2) & (mx[:, :, :, 0] > 0)).mean())


@pytest.mark.parametrize("H,W,csize", [(8, 8, 128), (6, 10, 128), (6, 10, 4), (8, 8, 16)])
@pytest.mark.parametrize("C", [4, 8, 48, 256, 1024])
def test_bwd_reduce_pooled(L, C, H, W, csize):
    rng = np.random.default_rng(C * 77 + H * W + csize)
    N = 3
    y = tie_y(rng, (N, H, W, C)); g = dyad(rng, (N, H // 2, W // 2, C))
    for gn in ([False, True] if C % 8 == 0 else [False]):
        np_ = _norm_params(rng, N, C, gn)
        assert tie_share(y, np_["s"], np_["t"]) >= 0.05
        got = _run_bwd_reduce(L, 1, g, y, np_, None, 0, csize, False)
        _, _, _, terms, mags = bwd_ref(1, g, y, np_["s"], np_["t"], np_["mean"], np_["invstd"], np_["cpg"], None)
        _check_bwd_slab(got, terms, mags, C, csize, 4, f"bwd_reduce pooled gn={gn}")


@pytest.mark.parametrize("C", [6, 1028, 0])
def test_reducers_reject_bad_C(L, C):
    """C % 4 != 0, C > 1024 and C < 4 are refused on the host: nothing is launched, the slab keeps its sentinel."""
    N, H, W = 2, 4, 4
    Ca = max(C, 8)
    y = T(np.ones((N, H, W, Ca))); g = T(np.ones((N, H, W, Ca)))
    v = T(np.ones((N, Ca)))
    slab = Z(N, 1, 5, Ca)
    ymm = Z(2, Ca, fill=0, dtype=torch.int32)
    E = _err()
    with pytest.raises(E):
        L.cdm_reduce_stats(P(y), Ca, N, H * W, C, 128, P(slab), _s())
    with pytest.raises(E):
        L.cdm_reduce_sum(P(y), Ca, N, H * W, C, 128, P(slab), _s())
    with pytest.raises(E):
        L.cdm_reduce_stats_mm(P(y), Ca, N, H * W, C, 128, P(slab), P(ymm), Ca, _s())
    for mode in (0, 1, 2):
        with pytest.raises(E):
            L.cdm_norm_bwd_reduce(mode, P(g), Ca, P(y), Ca, N, H, W, C, P(v), P(v), 0, P(v), P(v), 0, 1, P(v), 0, 128,
                                  P(slab), _s())
    assert bool((Hh(slab) == SENT).all()) and bool((Hh(ymm) == 0).all())


# ----------------------------------------------------------------------------------------------------------------
# cdm_reduce_stats_mm
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 8, 11, 17])
@pytest.mark.parametrize("C,csize", [(8, 16), (48, 200), (256, 40), (1024, 19)])
def test_reduce_stats_mm(L, C, csize, nch):
    rng = np.random.default_rng(C + nch)
    N = 2
    HW = csize * nch if nch != 11 else csize * 10 + csize // 2 + 1      # 11 chunks, the last one ragged
    y = rng.standard_normal((N, HW, C)).astype(np.float32)
    y[:, :, 0] = -np.abs(y[:, :, 0]) - 0.25                              # all negative
    y[:, :, 1] = 1.375                                                   # constant
    y[:, :, 2] = np.where(rng.random((N, HW)) < 0.5, -np.abs(y[:, :, 2]) - 0.5, 0.0)   # max is a zero of either sign
    y[:, :, 3] = np.where(rng.random((N, HW)) < 0.5, np.abs(y[:, :, 3]) + 0.5, 0.0)    # min is a zero of either sign
    y[0, 0, 2:4] = -0.0; y[-1, -1, 2:4] = 0.0; y[0, HW // 2, 2:4] = [0.0, -0.0]
    ld, off = C + 4, 4
    yd = T(widen(y.astype(np.float64), ld, off))
    yd[..., off:off + C] = torch.from_numpy(y).to(DEV)                   # keep the sign of -0.0
    ref_slab = Z(N, nch, 2, C)
    L.cdm_reduce_stats(P(yd, off), ld, N, HW, C, csize, P(ref_slab), _s())
    ymm_ld = C + 4
    keys = np.empty((2, ymm_ld), dtype=np.int32); keys[0] = np.iinfo(np.int32).min; keys[1] = np.iinfo(np.int32).max
    wide_c = [5, 6] if C > 6 else []
    keys[0, wide_c] = fkey(np.float32(100.0)); keys[1, wide_c] = fkey(np.float32(-100.0))
    ymm = T(keys, torch.int32)
    slab = Z(N, nch, 2, C)
    L.cdm_reduce_stats_mm(P(yd, off), ld, N, HW, C, csize, P(slab), P(ymm), ymm_ld, _s())
    _sync()
    assert torch.equal(slab, ref_slab), "slab differs from cdm_reduce_stats"
    # and that slab is right (so the pair cannot be wrong together)
    y64 = y.astype(np.float64)
    k = n_add(C, csize) + 8
    got = Hh(slab)
    check(got[:, :, 0], chunk_sums(y64, csize), k * U * chunk_sums(np.abs(y64), csize), "stats_mm sum")
    check(got[:, :, 1], chunk_sums(y64 * y64, csize), k * U * chunk_sums(y64 * y64, csize), "stats_mm sumsq")
    kk = ymm.cpu().numpy()
    mx, mn = y64.max(axis=(0, 1)), y64.min(axis=(0, 1))
    mx[wide_c] = 100.0; mn[wide_c] = -100.0
    exact(fkey_inv(kk[0, :C]), mx, "max keys"); exact(fkey_inv(kk[1, :C]), mn, "min keys")
    assert (kk[0, C:] == np.iinfo(np.int32).min).all() and (kk[1, C:] == np.iinfo(np.int32).max).all()
    slab2 = Z(N, nch, 2, C)
    L.cdm_reduce_stats_mm(P(yd, off), ld, N, HW, C, csize, P(slab2), None, 0, _s())      # ymm == NULL: slab only
    _sync()
    assert torch.equal(slab2, ref_slab)


# ----------------------------------------------------------------------------------------------------------------
# cdm_slab_colsum
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 64, 100])
def test_slab_colsum(L, C):
    rng = np.random.default_rng(C)
    for ntiles in (1, 3, 33, 70):
        for R in (1, 2, 5):
            slab = rng.standard_normal((ntiles, R, C)).astype(np.float32).astype(np.float64) * 8
            sd = T(slab)
            for splits in (1, 4, ntiles + 3):
                part = Z(splits, R, C, fill=float("nan"), dtype=torch.float64)
                L.cdm_slab_colsum(P(sd), ntiles, R, C, P(part), splits, _s())
                per = -(-ntiles // splits)
                ref = np.zeros((splits, R, C)); mag = np.zeros((splits, R, C))
                for sp in range(splits):
                    ref[sp] = slab[sp * per:(sp + 1) * per].sum(axis=0)
                    mag[sp] = np.abs(slab[sp * per:(sp + 1) * per]).sum(axis=0)
                what = f"colsum ntiles={ntiles} R={R} splits={splits}"
                check(Hh(part), ref, 2.0 ** -50 * mag, what)
                if per * (splits - 1) >= ntiles:
                    assert (Hh(part)[-1] == 0).all(), what + ": empty split not zero"


# ----------------------------------------------------------------------------------------------------------------
# BatchNorm finalizes
# ----------------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _bn_fwd_ref(part, count, gamma, beta):
    """mean, invstd, scale, shift, biased var from fp64 partials [S][R][C] (extended precision)"""
    s = _ld(part[:, 0]).sum(axis=0); q = _ld(part[:, 1]).sum(axis=0)
    mu = s / count
    var = np.maximum(q / count - mu * mu, 0)
    is_ = 1 / np.sqrt(var + _ld(EPS))
    sc = _ld(gamma) * is_
    return [np.asarray(a, dtype=np.float64) for a in (mu, is_, sc, _ld(beta) - mu * sc, var)]


def _check_bn_coeffs(mean, invstd, scale, shift, ref, beta, what, k=(1, 1, 2, 2)):
    mu, is_, sc, sh, _ = ref
    check(Hh(mean), mu, k[0] * ulp(mu), what + " mean")
    check(Hh(invstd), is_, k[1] * ulp(is_), what + " invstd")
    check(Hh(scale), sc, k[2] * ulp(sc), what + " scale")
    check(Hh(shift), sh, k[3] * ulp(np.maximum(np.abs(beta), np.abs(mu * sc))), what + " shift")


@pytest.mark.parametrize("S", [1, 15, 16, 17, 65, 130])
@pytest.mark.parametrize("C", [4, 16, 20, 130])
def test_bn_fwd_finalize(L, C, S):
    """against torch.nn.BatchNorm2d in fp64 on the (dyadic) data the partials came from: S partials of 3 pixels"""
    rng = np.random.default_rng(C * 131 + S)
    ppp = 3
    x = dyad(rng, (S, ppp, C))
    x[:, :, 1] = 2.5                                                   # constant channel: var clamps at 0
    count = S * ppp
    for R in (2, 5):
        part = np.full((S, R, C), np.nan)
        part[:, 0] = x.sum(axis=1); part[:, 1] = (x * x).sum(axis=1)
        gamma = coef(rng, C); beta = coef(rng, C)
        rm0 = rng.standard_normal(C).astype(np.float32).astype(np.float64)
        rv0 = (rng.random(C) + 0.5).astype(np.float32).astype(np.float64)
        bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=0.1).double().train()
        with torch.no_grad():
            bn.running_mean.copy_(torch.from_numpy(rm0)); bn.running_var.copy_(torch.from_numpy(rv0))
            bn(torch.from_numpy(x.reshape(1, count, 1, C)).permute(0, 3, 1, 2))
        ref = _bn_fwd_ref(part, count, gamma, beta)
        pd = T(part, torch.float64); gd = T(gamma); bd = T(beta)
        rm = T(rm0); rv = T(rv0); nbt = T(np.array([41]), torch.int64)
        out = [Z(C) for _ in range(4)]
        for call in range(2):
            if call == 1:                                             # a second call from the same running state
                rm = T(rm0); rv = T(rv0)
            L.cdm_bn_fwd_finalize(P(pd), S, R, C, float(count), P(gd), P(bd), P(rm), P(rv), P(nbt), 0.1, EPS,
                                  *[P(o) for o in out], None, 0, None, _s())
            what = f"bn_fwd_finalize R={R} call={call}"
            _check_bn_coeffs(*out, ref, beta, what)
            assert Hh(out[1])[1] == float(np.float32(1.0 / math.sqrt(EPS))), "constant channel: invstd != 1/sqrt(eps)"
            check(Hh(rm), bn.running_mean.numpy(), ulp(bn.running_mean.numpy()), what + " running_mean")
            check(Hh(rv), bn.running_var.numpy(), ulp(bn.running_var.numpy()), what + " running_var")
            assert int(nbt.item()) == 42 + call, "num_batches_tracked must rise by exactly 1 per call"
        # null running pointers and a null counter: the coefficients are unchanged
        out2 = [Z(C) for _ in range(4)]
        L.cdm_bn_fwd_finalize(P(pd), S, R, C, float(count), P(gd), P(bd), None, None, None, 0.1, EPS,
                              *[P(o) for o in out2], None, 0, None, _s())
        _sync()
        for a, b in zip(out, out2):
            assert torch.equal(a, b)


def test_bn_fwd_finalize_count_one(L):
    """one pixel: mean = y, var = 0, invstd = 1/sqrt(eps); the running variance takes the biased value (no n/(n-1))"""
    rng = np.random.default_rng(5)
    C = 20
    x = dyad(rng, (1, C))
    part = np.stack([x, x * x], axis=1)
    gamma = coef(rng, C); beta = coef(rng, C)
    rm0 = dyad(rng, C); rv0 = dyad(rng, C) + 5.0
    rm = T(rm0); rv = T(rv0); nbt = T(np.array([0]), torch.int64)
    out = [Z(C) for _ in range(4)]
    L.cdm_bn_fwd_finalize(P(T(part, torch.float64)), 1, 2, C, 1.0, P(T(gamma)), P(T(beta)), P(rm), P(rv), P(nbt), 0.1,
                          EPS, *[P(o) for o in out], None, 0, None, _s())
    _check_bn_coeffs(*out, _bn_fwd_ref(part, 1, gamma, beta), beta, "count 1")
    exact(Hh(out[0]), x[0], "count 1 mean")
    exact(Hh(out[1]), np.full(C, float(np.float32(1.0 / math.sqrt(EPS)))), "count 1 invstd")
    m = 0.1
    check(Hh(rm), m * x[0] + (1 - m) * rm0, ulp(m * x[0] + (1 - m) * rm0), "count 1 running_mean")
    check(Hh(rv), (1 - m) * rv0, ulp((1 - m) * rv0), "count 1 running_var")
    assert int(nbt.item()) == 1


def _ymm_case(rng, C):
    ymax = np.abs(dyad(rng, C)) + 0.5; ymin = -np.abs(dyad(rng, C)) - 1.0
    ld = C + 4
    keys = np.zeros((2, ld), dtype=np.int32); keys[0, :C] = fkey(ymax); keys[1, :C] = fkey(ymin)
    return ymax, ymin, keys, ld


def _check_amax_z(am, seed, scale, shift, gamma_sign, ymax, ymin, what):
    """the kernel's own (separately checked) fp32 scale / shift: z = relu(fmaf(y*, scale, shift)) with y* the max of
    y where scale >= 0 and the min where it is negative; scale = 0 leaves relu(shift)"""
    sc, sh = Hh(scale), Hh(shift)
    assert (np.sign(sc) == gamma_sign).all()
    yx = np.where(sc >= 0, ymax, ymin)
    z = np.maximum(fma32(yx, sc, sh).astype(np.float64), 0.0)
    if (gamma_sign == 0).all():
        exact(z, np.maximum(sh, 0.0), what + " relu(shift)")
    want = max(float(z.max()), seed)
    got = float(Hh(am)[0])
    assert abs(got - want) <= float(ulp(want)), f"{what}: amax_z {got!r}, want {want!r}"
    other = np.maximum(fma32(np.where(sc >= 0, ymin, ymax), sc, sh).astype(np.float64), 0.0)
    if seed == 0.0 and gamma_sign.any():
        assert abs(float(other.max()) - want) > 4 * float(ulp(want)), "test input does not tell the two keys apart"


@pytest.mark.parametrize("sign", [1, -1, 0])
@pytest.mark.parametrize("frozen", [False, True])
def test_bn_fwd_ymm(L, frozen, sign):
    rng = np.random.default_rng(11 + sign)
    C, S = 20, 5
    x = dyad(rng, (S, 4, C))
    part = np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)
    gamma = sign * (np.abs(coef(rng, C)) + 0.25); beta = np.abs(coef(rng, C)) + 0.25
    rmean = dyad(rng, C, lim=1.0); rvar = np.abs(dyad(rng, C)) + 0.5
    ymax, ymin, keys, ld = _ymm_case(rng, C)
    for seed in (0.0, 1000.0):                                        # amax_z is a running max
        am = T(np.array([seed])); out = [Z(C) for _ in range(4)]
        if frozen:
            L.cdm_bn_fwd_frozen(C, P(T(gamma)), P(T(beta)), P(T(rmean)), P(T(rvar)), EPS, *[P(o) for o in out],
                                P(T(keys, torch.int32)), ld, P(am), _s())
        else:
            L.cdm_bn_fwd_finalize(P(T(part, torch.float64)), S, 2, C, float(S * 4), P(T(gamma)), P(T(beta)), None, None,
                                  None, 0.1, EPS, *[P(o) for o in out], P(T(keys, torch.int32)), ld, P(am), _s())
        _check_amax_z(am, seed, out[2], out[3], np.full(C, float(sign)), ymax, ymin, f"frozen={frozen} sign={sign}")
    with pytest.raises(_err()):                                       # ymm without amax_z
        if frozen:
            L.cdm_bn_fwd_frozen(C, P(T(gamma)), P(T(beta)), P(T(rmean)), P(T(rvar)), EPS, *[P(o) for o in out],
                                P(T(keys, torch.int32)), ld, None, _s())
        else:
            L.cdm_bn_fwd_finalize(P(T(part, torch.float64)), S, 2, C, float(S * 4), P(T(gamma)), P(T(beta)), None, None,
                                  None, 0.1, EPS, *[P(o) for o in out], P(T(keys, torch.int32)), ld, None, _s())


@pytest.mark.parametrize("C", [4, 300])
def test_bn_eval_coeffs_and_frozen(L, C):
    """fp32 arithmetic throughout: invstd = 1 / sqrtf(rvar + eps) is three correctly rounded fp32 operations (the
    square root halves the error of the sum): <= 1.25 ulp, bound 2; scale one more rounding: 3; shift = beta - rmean
    scale inherits those and rounds twice more: 4 ulp of its largest term."""
    rng = np.random.default_rng(C)
    gamma = rng.standard_normal(C).astype(np.float32).astype(np.float64)
    beta = rng.standard_normal(C).astype(np.float32).astype(np.float64)
    rmean = rng.standard_normal(C).astype(np.float32).astype(np.float64)
    rvar = (rng.random(C) * 4 + 1e-3).astype(np.float32).astype(np.float64)
    is_ = 1 / np.sqrt(rvar + EPS); sc = gamma * is_
    ref = [rmean, is_, sc, beta - rmean * sc, rvar]
    args = [P(T(gamma)), P(T(beta)), P(T(rmean)), P(T(rvar)), EPS]
    out = [Z(C) for _ in range(4)]
    L.cdm_bn_eval_coeffs(C, *args, *[P(o) for o in out], _s())
    _check_bn_coeffs(*out, ref, beta, "bn_eval_coeffs", k=(0, 2, 3, 4))
    out2 = [Z(C) for _ in range(4)]
    L.cdm_bn_fwd_frozen(C, *args, *[P(o) for o in out2], None, 0, None, _s())
    _check_bn_coeffs(*out2, ref, beta, "bn_fwd_frozen", k=(0, 2, 3, 4))


@pytest.mark.parametrize("S", [1, 15, 16, 17, 65, 130])
@pytest.mark.parametrize("C", [4, 16, 20, 130])
def test_bn_bwd_finalize(L, C, S):
    rng = np.random.default_rng(C * 7 + S)
    part = dyad(rng, (S, 5, C)); part[:, 2:4] = np.nan                # rows 2, 3 are not this kernel's to read
    gamma = coef(rng, C); is_ = pow2(rng, C)
    count = float(S * 3)
    s1, s2, s5 = (_ld(part[:, r]).sum(axis=0) for r in (0, 1, 4))
    a = _ld(gamma * is_)
    f64 = lambda v: np.asarray(v, dtype=np.float64)   # noqa: E731
    for frozen in (False, True):
        b = 0 * a if frozen else -a * s1 / count
        cc = 0 * a if frozen else -a * s2 / count
        fn = L.cdm_bn_bwd_finalize_frozen if frozen else L.cdm_bn_bwd_finalize
        for with_dbias in (True, False):
            out = [Z(C) for _ in range(6)]                            # dgamma dbeta A B Cc dbias
            fn(P(T(part, torch.float64)), S, C, count, P(T(gamma)), P(T(is_)), *[P(o) for o in out[:5]],
               P(out[5]) if with_dbias else None, _s())
            what = f"bn_bwd_finalize frozen={frozen}"
            check(Hh(out[0]), f64(s2), ulp(f64(s2)), what + " dgamma"); check(Hh(out[1]), f64(s1), ulp(f64(s1)), what + " dbeta")
            check(Hh(out[2]), f64(a), ulp(f64(a)), what + " A")
            check(Hh(out[3]), f64(b), 2 * ulp(f64(b)), what + " B"); check(Hh(out[4]), f64(cc), 2 * ulp(f64(cc)), what + " Cc")
            if frozen:
                assert (Hh(out[3]) == 0).all() and (Hh(out[4]) == 0).all()
            if with_dbias:
                terms = np.maximum(np.maximum(np.abs(f64(a * s1)), np.abs(f64(b * count))), np.abs(f64(cc * s5)))
                check(Hh(out[5]), f64(a * s1 + b * count + cc * s5), 2 * ulp(terms), what + " dbias")
            else:
                assert (Hh(out[5]) == SENT).all()


# ----------------------------------------------------------------------------------------------------------------
# GroupNorm finalizes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 3, 40])
@pytest.mark.parametrize("cpg", [1, 2, 6, 16, 64])
def test_gn_finalizes(L, cpg, nch):
    rng = np.random.default_rng(cpg * 100 + nch)
    N, G, px = 3, 8, 8
    C = G * cpg
    x = dyad(rng, (N, nch, px, C)) + (np.arange(C) % 5 - 2)[None, None, None, :] * 0.5   # groups differ
    gamma = coef(rng, C); beta = coef(rng, C)
    count = float(nch * px * cpg)
    xg = _ld(x).reshape(N, nch * px, G, cpg)
    mu = xg.sum(axis=(1, 3)) / count
    var = np.maximum((xg * xg).sum(axis=(1, 3)) / count - mu * mu, 0)
    is_ = 1 / np.sqrt(var + _ld(EPS))
    sc = _ld(gamma)[None] * np.repeat(is_, cpg, axis=1)
    sh = _ld(beta)[None] - np.repeat(mu, cpg, axis=1) * sc
    f64 = lambda v: np.asarray(v, dtype=np.float64)   # noqa: E731
    for R in (2, 5):
        slab = np.full((N, nch, R, C), np.nan)
        slab[:, :, 0] = x.sum(axis=2); slab[:, :, 1] = (x * x).sum(axis=2)     # exact in fp32 (dyadic, 8 pixels)
        mean, invstd, scale, shift = Z(N, G), Z(N, G), Z(N, C), Z(N, C)
        L.cdm_gn_fwd_finalize(P(T(slab)), N, nch, R, C, G, count, P(T(gamma)), P(T(beta)), EPS, P(mean), P(invstd),
                              P(scale), P(shift), _s())
        check(Hh(mean), f64(mu), ulp(f64(mu)), "gn_fwd mean"); check(Hh(invstd), f64(is_), ulp(f64(is_)), "gn_fwd invstd")
        check(Hh(scale), f64(sc), 2 * ulp(f64(sc)), "gn_fwd scale")
        big = np.maximum(np.abs(beta)[None], np.abs(f64(np.repeat(mu, cpg, axis=1) * sc)))
        check(Hh(shift), f64(sh), 2 * ulp(big), "gn_fwd shift")
    # backward: dy = A gpre + B + Cc xhat with dxhat = gamma gpre,
    # dy = invstd (dxhat - mean_g(dxhat) - xhat mean_g(dxhat xhat))  (mean_g over the group's cpg HW elements)
    HW = nch * px
    slab = dyad(rng, (N, nch, 5, C)); slab[:, :, 2:4] = np.nan
    isb = pow2(rng, (N, G))
    ch1, ch2, ch5 = (_ld(slab[:, :, r]).sum(axis=1) for r in (0, 1, 4))             # [N, C]
    isc = _ld(np.repeat(isb, cpg, axis=1))
    grp = lambda v: np.repeat((_ld(gamma)[None] * v).reshape(N, G, cpg).sum(axis=2), cpg, axis=1)   # noqa: E731
    a = _ld(gamma)[None] * isc
    b = -isc * grp(ch1) / count; cc = -isc * grp(ch2) / count
    out = [Z(N, C) for _ in range(6)]                                               # A B Cc pdg pdb pdbias
    L.cdm_gn_bwd_finalize(P(T(slab)), N, nch, C, G, count, HW, P(T(gamma)), P(T(isb)), *[P(o) for o in out], _s())
    check(Hh(out[0]), f64(a), ulp(f64(a)), "gn_bwd A")
    check(Hh(out[1]), f64(b), 2 * ulp(f64(b)), "gn_bwd B"); check(Hh(out[2]), f64(cc), 2 * ulp(f64(cc)), "gn_bwd Cc")
    check(Hh(out[3]), f64(ch2), ulp(f64(ch2)), "gn_bwd pdg"); check(Hh(out[4]), f64(ch1), ulp(f64(ch1)), "gn_bwd pdb")
    terms = np.maximum(np.maximum(np.abs(f64(a * ch1)), np.abs(f64(b * HW))), np.abs(f64(cc * ch5)))
    check(Hh(out[5]), f64(a * ch1 + b * HW + cc * ch5), 2 * ulp(terms), "gn_bwd pdbias")


def test_gn_finalizes_reject(L):
    E = _err()
    N, nch = 1, 1
    for C, G, fwd_bad, bwd_bad in [(20, 8, True, True), (130, 65, True, False), (520, 8, False, True)]:
        slab = T(np.ones((N, nch, 5, C))); v = T(np.ones((N, C)))
        outs = [Z(N, C) for _ in range(6)]
        if fwd_bad:
            with pytest.raises(E):
                L.cdm_gn_fwd_finalize(P(slab), N, nch, 5, C, G, 1.0, P(v), P(v), EPS, *[P(o) for o in outs[:4]], _s())
        if bwd_bad:
            with pytest.raises(E):
                L.cdm_gn_bwd_finalize(P(slab), N, nch, C, G, 1.0, 1, P(v), P(v), *[P(o) for o in outs], _s())
        assert all(bool((Hh(o) == SENT).all()) for o in outs)


# ----------------------------------------------------------------------------------------------------------------
# elementwise applies
# ----------------------------------------------------------------------------------------------------------------
def apply_fwd_ref(flags, y, s, t, fa, fb, rx, rw, rb, rsplit):
    N = y.shape[0]
    z = y * bc(s) + bc(t)
    if flags & 8:
        z = np.maximum(z, 0.0)
    if flags & 1:
        z = win(z).max(axis=3)
    if flags & 2:
        z = bc(fa) * z + bc(fb)
    if flags & 4:
        sel = (np.arange(N) >= rsplit).astype(int)
        if rx.ndim == 3:
            z = bc(rw[sel]) * rx[..., None] + bc(rb[sel]) + z
        else:
            z = np.einsum("nck,nhwk->nhwc", rw[sel], rx) + bc(rb[sel]) + z
    return z


def _run_apply_fwd(L, flags, y, s, t, sn, fa, fb, fan, fbn, rx, rw, rb, rsplit, wide, seed):
    N, H, W, C = y.shape
    Ho, Wo = (H // 2, W // 2) if flags & 1 else (H, W)
    ldy, offy = (C + 8, 4) if wide else (C, 0)
    ldo, offo = (C + 12, 8) if wide else (C, 0)
    out = Z(N, Ho, Wo, ldo); am = T(np.array([seed]))
    opt = lambda a: None if a is None else T(a)   # noqa: E731
    L.cdm_norm_apply_fwd(flags, P(T(widen(y, ldy, offy)), offy), ldy, N, H, W, C, P(T(s)), P(T(t)), sn, P(opt(fa)), fan,
                         P(opt(fb)), fbn, P(opt(rx)), P(opt(rw)), P(opt(rb)), rsplit, P(out, offo), ldo, P(am), _s())
    o = Hh(out)
    assert (np.delete(o, np.s_[offo:offo + C], axis=-1) == SENT).all(), "wrote outside its channel slice"
    return o[..., offo:offo + C], float(Hh(am)[0])


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("flags", [0, 8, 1, 9, 2, 10, 4, 12])
def test_norm_apply_fwd(L, flags, wide, per_sample):
    rng = np.random.default_rng(flags * 4 + wide * 2 + per_sample)
    N, H, W, C = 3, 6, 10, 12
    y = tie_y(rng, (N, H, W, C)) if flags & 1 else dyad(rng, (N, H, W, C))
    Ns = N if per_sample else 1
    s, t = coef(rng, (Ns, C)), coef(rng, (Ns, C))
    if flags & 1:
        assert tie_share(y, s, t) >= 0.05
    fa = fb = rx = None
    if flags & 2:
        fa, fb = coef(rng, (Ns, C)), coef(rng, (Ns, C))
    if flags & 4:
        rx = dyad(rng, (N, H, W))
    for rsplit in ((1, N, N + 2) if flags & 4 else (N,)):
        rw = rb = None
        if flags & 4:                                                 # one draw only when no sample takes the second
            nd = 2 if rsplit < N else 1
            rw, rb = coef(rng, (nd, C)), coef(rng, (nd, C))
        for seed in (0.0, 64.0):
            got, am = _run_apply_fwd(L, flags, y, s, t, C if per_sample else 0, fa, fb, C if per_sample else 0,
                                     C if per_sample else 0, rx, rw, rb, rsplit, wide, seed)
            ref = apply_fwd_ref(flags, y, s, t, fa, fb, rx, rw, rb, rsplit)
            exact(got, ref, f"apply_fwd flags={flags} rsplit={rsplit}")
            assert am == max(seed, float(np.abs(ref).max()))


def test_norm_apply_fwd_rejects(L):
    E = _err()
    N, H, W, C = 1, 2, 2, 8
    y = T(np.ones((N, H, W, C))); v = T(np.ones((2, C))); x = T(np.ones((N, H, W))); out = Z(N, H, W, C)
    for flags, Cc in [(1 | 2, C), (1 | 4, C), (2 | 4, C), (1 | 2 | 8, C), (8, 6)]:
        with pytest.raises(E):
            L.cdm_norm_apply_fwd(flags, P(y), C, N, H, W, Cc, P(v), P(v), 0, P(v), 0, P(v), 0, P(x), P(v), P(v), N, P(out),
                                 C, None, _s())
    with pytest.raises(E):
        L.cdm_norm_apply_fwd_resid_c(1, P(y), C, N, H, W, 6, P(v), P(v), P(x), 1, 1, P(v), P(v), N, P(out), C, None, _s())
    with pytest.raises(E):
        L.cdm_norm_apply_bwd(0, P(y), C, P(y), C, N, H, W, 6, P(v), P(v), 0, P(v), P(v), 0, 1, None, 0, P(v), P(v), P(v),
                             0, P(out), C, None, _s())
    assert bool((Hh(out) == SENT).all())


@pytest.fixture(scope="module")
def big():
    """N = 3, 128 x 128, C = 256: 3.1 M float4 items against the 8192 x 256 threads of the capped grid"""
    rng = np.random.default_rng(2024)
    N, H, W, C = 3, 128, 128, 256
    d = dict(N=N, H=H, W=W, C=C, y=dyad(rng, (N, H, W, C)).astype(np.float32),
             g=dyad(rng, (N, H, W, C)).astype(np.float32))
    for k in ("s", "t", "A", "B", "Cc"):
        d[k] = coef(rng, (1, C))
    d["invstd"] = pow2(rng, (1, C))
    return d


def test_norm_apply_fwd_grid_stride(L, big):
    N, H, W, C = big["N"], big["H"], big["W"], big["C"]
    assert N * H * W * (C // 4) > 8192 * 256
    out = Z(N, H, W, C); am = T(np.array([0.0]))
    L.cdm_norm_apply_fwd(8, P(T(big["y"])), C, N, H, W, C, P(T(big["s"])), P(T(big["t"])), 0, None, 0, None, 0, None, None,
                         None, N, P(out), C, P(am), _s())
    _sync()
    ref = np.maximum(big["y"] * bc(big["s"]).astype(np.float32) + bc(big["t"]).astype(np.float32), np.float32(0))
    assert ref.dtype == np.float32                                     # exact in fp32 on dyadic inputs
    assert np.array_equal(out.cpu().numpy(), ref)
    assert float(am.item()) == float(np.abs(ref).max())


@pytest.mark.parametrize("rsplit", [1, 5])
@pytest.mark.parametrize("xc,ldx", [(2, 2), (3, 5), (16, 16), (16, 20)])
def test_norm_apply_fwd_resid_c(L, xc, ldx, rsplit):
    rng = np.random.default_rng(xc * 10 + ldx + rsplit)
    N, H, W, C = 3, 5, 7, 12
    y = dyad(rng, (N, H, W, C)); s, t = coef(rng, (1, C)), coef(rng, (1, C))
    rx = dyad(rng, (N, H, W, xc))
    nd = 2 if rsplit < N else 1
    rw, rb = coef(rng, (nd, C, xc)), coef(rng, (nd, C))
    ldy, ldo = C + 4, C + 8
    for relu in (0, 1):
        out = Z(N, H, W, ldo); am = T(np.array([0.0]))
        L.cdm_norm_apply_fwd_resid_c(relu, P(T(widen(y, ldy, 4)), 4), ldy, N, H, W, C, P(T(s)), P(T(t)),
                                     P(T(widen(rx, ldx, 0))), ldx, xc, P(T(rw)), P(T(rb)), rsplit, P(out, 4), ldo, P(am),
                                     _s())
        ref = apply_fwd_ref(4 | (8 if relu else 0), y, s, t, None, None, rx, rw, rb, rsplit)
        o = Hh(out)
        exact(o[..., 4:4 + C], ref, f"resid_c xc={xc} relu={relu}")
        assert (np.delete(o, np.s_[4:4 + C], axis=-1) == SENT).all()
        assert float(Hh(am)[0]) == float(np.abs(ref).max())


@pytest.mark.parametrize("cn_per_sample", [False, True])
@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_norm_apply_bwd(L, mode, gn, cn_per_sample):
    rng = np.random.default_rng(mode * 4 + gn * 2 + cn_per_sample)
    N, H, W, C = 3, 6, 10, 24
    y = tie_y(rng, (N, H, W, C)) if mode == 1 else dyad(rng, (N, H, W, C))
    g = dyad(rng, (N, H // 2, W // 2, C) if mode == 1 else (N, H, W, C))
    np_ = _norm_params(rng, N, C, gn)
    if mode == 1:
        assert tie_share(y, np_["s"], np_["t"]) >= 0.05
    fa = coef(rng, (N, C)) if mode == 2 else None
    Nc = N if cn_per_sample else 1
    A, B, Cc = coef(rng, (Nc, C)), coef(rng, (Nc, C)), coef(rng, (Nc, C))
    gpre, xh, _, _, _ = bwd_ref(mode, g, y, np_["s"], np_["t"], np_["mean"], np_["invstd"], np_["cpg"], fa)
    ref = bc(Cc) * xh + (bc(A) * gpre + bc(B))
    ldg, ldy, ldd = C + 4, C + 8, C + 12
    for seed in (0.0, 4096.0):
        dy = Z(N, H, W, ldd); am = T(np.array([seed]))
        L.cdm_norm_apply_bwd(mode, P(T(widen(g, ldg, 4)), 4), ldg, P(T(widen(y, ldy, 4)), 4), ldy, N, H, W, C,
                             P(T(np_["s"])), P(T(np_["t"])), np_["sn"], P(T(np_["mean"])), P(T(np_["invstd"])), np_["mn"],
                             np_["cpg"], P(T(fa)) if fa is not None else None, C, P(T(A)), P(T(B)), P(T(Cc)),
                             C if cn_per_sample else 0, P(dy, 8), ldd, P(am), _s())
        o = Hh(dy)
        exact(o[..., 8:8 + C], ref, f"apply_bwd mode={mode} gn={gn}")
        assert (np.delete(o, np.s_[8:8 + C], axis=-1) == SENT).all()
        assert float(Hh(am)[0]) == max(seed, float(np.abs(ref).max()))


def test_norm_apply_bwd_grid_stride(L, big):
    N, H, W, C = big["N"], big["H"], big["W"], big["C"]
    dy = Z(N, H, W, C)
    f = lambda k: T(big[k])   # noqa: E731
    L.cdm_norm_apply_bwd(0, P(f("g")), C, P(f("y")), C, N, H, W, C, P(f("s")), P(f("t")), 0, P(T(np.zeros((1, C)))),
                         P(f("invstd")), 0, 1, None, 0, P(f("A")), P(f("B")), P(f("Cc")), 0, P(dy), C, None, _s())
    _sync()
    c32 = lambda k: bc(big[k]).astype(np.float32)   # noqa: E731
    zp = big["y"] * c32("s") + c32("t")
    ref = c32("Cc") * (big["y"] * c32("invstd")) + (c32("A") * np.where(zp > 0, big["g"], np.float32(0)) + c32("B"))
    assert ref.dtype == np.float32                                     # every step exact in fp32 on dyadic inputs
    assert np.array_equal(dy.cpu().numpy(), ref)


# ----------------------------------------------------------------------------------------------------------------
# the small folds
# ----------------------------------------------------------------------------------------------------------------
def test_slab_sum_nc(L):
    rng = np.random.default_rng(3)
    for N, nch, R, C in [(3, 1, 5, 48), (2, 7, 5, 100), (3, 40, 2, 4)]:
        slab = dyad(rng, (N, nch, R, C))
        for r in range(R):
            out = Z(N, C)
            L.cdm_slab_sum_nc(P(T(slab)), N, nch, R, r, C, P(out), _s())
            ref = slab[:, :, r].sum(axis=1)
            check(Hh(out), ref, ulp(ref), f"slab_sum_nc r={r}")


@pytest.mark.parametrize("S", [1, 3, 4, 9])
def test_slab_sum_all(L, S):
    rng = np.random.default_rng(S)
    R, C = 10, 20
    part = dyad(rng, (S, R, C))
    pd = T(part, torch.float64)
    tot = part.sum(axis=0)                                             # [R][C]
    for r0, rn, s_r, s_c in [(0, 9, 1, 9), (9, 1, 0, 1), (2, 3, C, 1), (0, 10, C, 1)]:
        idx = (np.arange(rn)[:, None] * s_r + np.arange(C)[None, :] * s_c)
        n_out = int(idx.max()) + 1
        for acc in (0, 1):
            init = dyad(rng, n_out + 5)
            out = T(init)
            L.cdm_slab_sum_all(P(pd), S, R, r0, rn, C, P(out), s_r, s_c, acc, _s())
            ref = init.copy()
            ref[idx] = (init[idx] if acc else 0.0) + tot[r0:r0 + rn]
            check(Hh(out), ref, ulp(ref) * (np.isin(np.arange(n_out + 5), idx)), f"slab_sum_all r0={r0} rn={rn} acc={acc}")


@pytest.mark.parametrize("N", [1, 4, 33, 70])
@pytest.mark.parametrize("C", [1, 64, 100])
def test_col_sum(L, C, N):
    rng = np.random.default_rng(C * 100 + N)
    ins = [dyad(rng, (N, C)) for _ in range(3)]
    refs = [a.sum(axis=0) for a in ins]
    for acc in (0, 1):
        init = dyad(rng, C + 3)
        out = T(init)
        L.cdm_col_sum(P(T(ins[0])), N, C, P(out), acc, _s())
        ref = init.copy(); ref[:C] = (init[:C] if acc else 0.0) + refs[0]
        exact(Hh(out), ref, f"col_sum acc={acc}")                      # dyadic: every sum is exact
    for k in (1, 2, 3):
        outs = [Z(C + 3) for _ in range(3)]
        a = []
        for j in range(3):
            a += [P(T(ins[j])), P(outs[j])] if j < k else [None, None]
        L.cdm_col_sum3(*a, N, C, _s())
        for j in range(3):
            ref = np.full(C + 3, SENT)
            if j < k:
                ref[:C] = refs[j]
            exact(Hh(outs[j]), ref, f"col_sum3 pairs={k} out{j}")


def test_col_sum3_rejects(L):
    """in2 without in1, and an input without its output, are refused before a launch"""
    N, C = 4, 8
    a = T(np.ones((N, C))); o = [Z(C) for _ in range(3)]
    E = _err()
    for args in [(P(a), P(o[0]), None, None, P(a), P(o[2])),
                 (P(a), P(o[0]), None, P(o[1]), P(a), P(o[2])),
                 (P(a), None, None, None, None, None),
                 (P(a), P(o[0]), P(a), None, None, None),
                 (P(a), P(o[0]), P(a), P(o[1]), P(a), None)]:
        with pytest.raises(E):
            L.cdm_col_sum3(*args, N, C, _s())
    assert all(bool((Hh(x) == SENT).all()) for x in o)


@pytest.mark.parametrize("n", [0, 1, 300, 2 ** 20 + 3])
def test_fill_i32(L, n):
    buf = Z(n + 7, fill=-5, dtype=torch.int32)
    L.cdm_fill_i32(P(buf), n, 123456789, _s())
    _sync()
    b = buf.cpu().numpy()
    assert (b[:n] == 123456789).all() and (b[n:] == -5).all()


@pytest.mark.parametrize("side", [4, 3])
def test_avgpool_gelu(L, side):
    """to_vec = AvgPool2d(side) + exact GELU on a side x side map, and its autograd, in torch fp64.
    hpre = sums * (1.0f / HW): two fp32 roundings, 2 ulp.  hv = GELU in fp64 of that hpre, rounded once: |GELU'| <=
    1.13 carries hpre's error, plus the rounding.  Backward: the elementwise bound 4 u (sum of the magnitudes of the
    terms): |dst| + |dhv| / HW (1/2 + |erf(x / sqrt 2)| / 2 + |x| pdf(x)), the three terms of GELU'(x), which cancel
    for x < 0."""
    rng = np.random.default_rng(side)
    N, C, HW = 3, 20, side * side
    x = dyad(rng, (N, C, side, side))
    xt = torch.from_numpy(x).requires_grad_()
    hv_ref = torch.nn.GELU()(torch.nn.AvgPool2d(side)(xt))
    dhv = rng.standard_normal((N, C)).astype(np.float32).astype(np.float64)
    hv_ref.backward(torch.from_numpy(dhv).reshape(N, C, 1, 1))
    m_ref = x.mean(axis=(2, 3))
    hpre, hv = Z(N, C), Z(N, C)
    L.cdm_avgpool_gelu_fin(P(T(x.sum(axis=(2, 3)))), N, C, HW, P(hpre), P(hv), _s())
    check(Hh(hpre), m_ref, 2 * ulp(m_ref), "avgpool mean")
    hvr = hv_ref.detach().numpy().reshape(N, C)
    check(Hh(hv), hvr, 1.13 * 2 * ulp(m_ref) + ulp(hvr), "gelu")
    ld = C + 8
    init = dyad(rng, (N, side, side, ld))
    dst = T(init)
    L.cdm_avgpool_gelu_bwd(P(T(dhv)), P(T(m_ref)), N, HW, C, P(dst, 4), ld, _s())
    ref = init.copy()
    add = xt.grad.numpy().transpose(0, 2, 3, 1)
    ref[..., 4:4 + C] += add
    bound = np.zeros_like(ref)
    erf = torch.erf(torch.from_numpy(m_ref / math.sqrt(2.0))).numpy()
    pdf = np.exp(-0.5 * m_ref * m_ref) / math.sqrt(2.0 * math.pi)
    mags = np.abs(dhv) / HW * (0.5 + 0.5 * np.abs(erf) + np.abs(m_ref) * pdf)      # GELU' = 1/2 + erf/2 + x pdf
    bound[..., 4:4 + C] = 4 * U * (np.abs(init[..., 4:4 + C]) + mags[:, None, None, :])
    check(Hh(dst), ref, bound, "avgpool_gelu_bwd")


# ----------------------------------------------------------------------------------------------------------------
# end-to-end chains
# ----------------------------------------------------------------------------------------------------------------
def chain_bounds(y, gamma, beta, k, kb, gpre, gout=None, fa=None, fb=None):
    """First-order propagation of the reduction bound through a norm chain (u = 2^-24).

    y, gpre: [B, M, G, q] fp64 reference values (BatchNorm: B = 1, M = N HW, G = C, q = 1; GroupNorm: B = N, M = HW,
    q channels per group); gamma, beta [G, q].  Statistics are over (M, q); k = n_add + 8 of the forward reducer, kb
    of the backward one.
      sums:      d(sum y) <= k u sum|y|, d(sum y^2) <= k u sum y^2  (fp64 folds add nothing at this level)
      mean:      dmu = k u E|y|
      variance:  var = E[y^2] - mu^2, so dvar <= k u E[y^2] + 2 |mu| dmu   (the cancelling form: E[y^2], not var)
      invstd:    d invstd / invstd <= 1/2 dvar / (var + eps) =: rho (+ 2 u for the roundings)
      xhat:      dxh = |xh| rho + invstd dmu + 2 u |xh|
      scale s = gamma invstd:  ds = |s| (rho + 2 u);  shift t = beta - mu s:  dt = |s| dmu + |mu| ds + 2 u max term
      z = relu(y s + t):  dz = |y| ds + dt + 4 u (|y s| + |t|)     (same gate: asserted precondition)
      S1 = sum gpre, S2 = sum gpre xh, S5 = sum xh per channel: dS = kb u sum|term| + sum (term's own error)
      A = gamma invstd, B = -invstd sum_q(gamma S1) / n, Cc = -invstd sum_q(gamma S2) / n, each with rho + 2 u
      dy = A gpre + B + Cc xh:  ddy = dA |gpre| + dB + dCc |xh| + |Cc| dxh + 4 u (|A gpre| + |B| + |Cc xh|)
      dgamma = sum_b S2, dbeta = sum_b S1 (one more rounding each), dbias = sum_b (A S1 + B M + Cc S5)
      FiLM out = a u + b, da = sum g u, db = sum g: the same rules with du = dz
    """
    u = U
    Bn, M, G, q = y.shape
    n = M * q
    St = lambda a: a.sum(axis=(1, 3), keepdims=True)   # noqa: E731
    Sc = lambda a: a.sum(axis=1, keepdims=True)        # noqa: E731
    Sq = lambda a: a.sum(axis=3, keepdims=True)        # noqa: E731
    mu = St(y) / n; ey2 = St(y * y) / n
    var = ey2 - mu * mu
    is_ = 1 / np.sqrt(var + EPS)
    dmu = k * u * St(np.abs(y)) / n
    dvar = k * u * ey2 + 2 * np.abs(mu) * dmu
    rho = 0.5 * dvar / (var + EPS) + 2 * u
    xh = (y - mu) * is_
    dxh = np.abs(xh) * rho + is_ * dmu + 2 * u * np.abs(xh)
    s = gamma * is_; t = beta - mu * s
    ds = np.abs(s) * (rho + 2 * u)
    dt = np.abs(s) * dmu + np.abs(mu) * ds + 2 * u * np.maximum(np.abs(beta), np.abs(mu * s))
    dz = np.abs(y) * ds + dt + 4 * u * (np.abs(y * s) + np.abs(t))
    S1, S2, S5 = Sc(gpre), Sc(gpre * xh), Sc(xh)
    dS1 = kb * u * Sc(np.abs(gpre))
    dS2 = kb * u * Sc(np.abs(gpre * xh)) + Sc(np.abs(gpre) * dxh)
    dS5 = kb * u * Sc(np.abs(xh)) + Sc(dxh)
    A = gamma * is_; dA = np.abs(A) * (rho + 2 * u)
    B = -is_ * Sq(gamma * S1) / n; dB = is_ * Sq(np.abs(gamma) * dS1) / n + np.abs(B) * (rho + 2 * u)
    Cc = -is_ * Sq(gamma * S2) / n; dCc = is_ * Sq(np.abs(gamma) * dS2) / n + np.abs(Cc) * (rho + 2 * u)
    ddy = dA * np.abs(gpre) + dB + dCc * np.abs(xh) + np.abs(Cc) * dxh \
        + 4 * u * (np.abs(A * gpre) + np.abs(B) + np.abs(Cc * xh))
    fold = lambda d, v: (d + 2 * u * np.abs(v)).sum(axis=0).reshape(-1)   # noqa: E731
    dpb = dA * np.abs(S1) + np.abs(A) * dS1 + M * dB + dCc * np.abs(S5) + np.abs(Cc) * dS5 \
        + 2 * u * np.maximum(np.maximum(np.abs(A * S1), np.abs(B * M)), np.abs(Cc * S5))
    out = dict(rho=rho, invstd=is_, dz=np.broadcast_to(dz, y.shape), ddy=np.broadcast_to(ddy, y.shape),
               dgamma=fold(dS2, S2), dbeta=fold(dS1, S1), dbias=fold(dpb, A * S1))
    if gout is not None:
        uu = np.maximum(y * s + t, 0.0)
        out["dout"] = np.abs(fa) * dz + 4 * u * (np.abs(fa * uu) + np.abs(fb))
        out["dfa"] = (kb * u * Sc(np.abs(gout * uu)) + Sc(np.abs(gout) * dz) + u * np.abs(Sc(gout * uu)))[:, 0]
        out["dfb"] = (kb * u * Sc(np.abs(gout)) + u * np.abs(Sc(gout)))[:, 0]
    return out


def _gate_ok(y, s, t):
    zp = y * s + t
    return bool((np.abs(zp) >= 1e-6 * (np.abs(y * s) + np.abs(t))).all())


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def _bn_chain(L, seed, H, W, pool, shift_ratio=0.0):
    """the kernels of one BatchNorm layer, forward and backward, against fp64 torch autograd of
    y = x + bias; BatchNorm2d (train); ReLU; [MaxPool2d(2)]"""
    rng = np.random.default_rng(seed)
    N, C, csize = 3, 48, 128
    HW = H * W
    sig = 0.5 + rng.random(C)
    bias = rng.standard_normal(C).astype(np.float32)
    xc = (rng.standard_normal((N, H, W, C)) * sig).astype(np.float32)
    if shift_ratio:
        xc = (xc + np.where(np.arange(C) % 2 == 0, 1.0, -1.0) * shift_ratio * sig).astype(np.float32)
    y = (xc + bias).astype(np.float32)                                 # the conv output the kernels see
    y64 = y.astype(np.float64)
    gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32).astype(np.float64)
    beta = (0.5 * rng.standard_normal(C)).astype(np.float32).astype(np.float64)
    gshape = (N, H // 2, W // 2, C) if pool else (N, H, W, C)
    g = rng.standard_normal(gshape).astype(np.float32).astype(np.float64)
    # reference (x = y - bias exactly, so that x + bias is the y above)
    xt = (_nchw(y64) - torch.from_numpy(bias.astype(np.float64)).reshape(1, C, 1, 1)).requires_grad_()
    bt = torch.from_numpy(bias.astype(np.float64)).requires_grad_()
    bn = torch.nn.BatchNorm2d(C, eps=EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
    yt = xt + bt.reshape(1, C, 1, 1)
    yt.retain_grad()
    o = torch.relu(bn(yt))
    if pool:
        o = torch.nn.MaxPool2d(2)(o)
    o.backward(_nchw(g))
    mu = y64.mean(axis=(0, 1, 2)); var = y64.var(axis=(0, 1, 2)); is_ref = 1 / np.sqrt(var + EPS)
    s_ref = gamma * is_ref; t_ref = beta - mu * s_ref
    assert _gate_ok(y64, s_ref, t_ref), "seed precondition: a pre-activation within 1e-6 of the gate"
    mode = 1 if pool else 0
    gpre, _, _, _, _ = bwd_ref(mode, g, y64, s_ref[None], t_ref[None], mu[None], is_ref[None], 1, None)
    k = n_add(C, csize) + 8; kb = n_add(C, csize, 4 if pool else 1) + 8
    bd = chain_bounds(y64.reshape(1, N * HW, C, 1), gamma[:, None], beta[:, None], k, kb, gpre.reshape(1, N * HW, C, 1))
    # kernels, forward
    yd = T(y); nch = -(-HW // csize); splits = 4
    slab = Z(N, nch, 2, C); part = Z(splits, 2, C, dtype=torch.float64)
    L.cdm_reduce_stats(P(yd), C, N, HW, C, csize, P(slab), _s())
    L.cdm_slab_colsum(P(slab), N * nch, 2, C, P(part), splits, _s())
    mean, invstd, scale, shift = Z(C), Z(C), Z(C), Z(C)
    gd_, bd_ = T(gamma), T(beta)
    L.cdm_bn_fwd_finalize(P(part), splits, 2, C, float(N * HW), P(gd_), P(bd_), None, None, None, 0.1, EPS, P(mean),
                          P(invstd), P(scale), P(shift), None, 0, None, _s())
    out = Z(*gshape)
    L.cdm_norm_apply_fwd(8 | mode, P(yd), C, N, H, W, C, P(scale), P(shift), 0, None, 0, None, 0, None, None, None, N,
                         P(out), C, None, _s())
    rel_is = np.abs(Hh(invstd) - is_ref) / is_ref
    check(rel_is, 0 * rel_is, bd["rho"].reshape(-1), "chain invstd (relative)")
    dz = bd["dz"].reshape(N, H, W, C)
    check(Hh(out), _nhwc(o), win(dz).max(axis=3) if pool else dz, "chain output")
    # kernels, backward
    gdv = T(g); HWp = (H // 2) * (W // 2) if pool else HW
    nchb = -(-HWp // csize)
    slab5 = Z(N, nchb, 5, C); part5 = Z(splits, 5, C, dtype=torch.float64)
    L.cdm_norm_bwd_reduce(mode, P(gdv), C, P(yd), C, N, H, W, C, P(scale), P(shift), 0, P(mean), P(invstd), 0, 1, None, 0,
                          csize, P(slab5), _s())
    L.cdm_slab_colsum(P(slab5), N * nchb, 5, C, P(part5), splits, _s())
    o6 = [Z(C) for _ in range(6)]                                      # dgamma dbeta A B Cc dbias
    L.cdm_bn_bwd_finalize(P(part5), splits, C, float(N * HW), P(gd_), P(invstd), *[P(v) for v in o6], _s())
    dy = Z(N, H, W, C)
    L.cdm_norm_apply_bwd(mode, P(gdv), C, P(yd), C, N, H, W, C, P(scale), P(shift), 0, P(mean), P(invstd), 0, 1, None, 0,
                         P(o6[2]), P(o6[3]), P(o6[4]), 0, P(dy), C, None, _s())
    check(Hh(dy), _nhwc(yt.grad), bd["ddy"].reshape(N, H, W, C), "chain dy")
    check(Hh(o6[0]), bn.weight.grad.numpy(), bd["dgamma"], "chain dgamma")
    check(Hh(o6[1]), bn.bias.grad.numpy(), bd["dbeta"], "chain dbeta")
    check(Hh(o6[5]), bt.grad.numpy(), bd["dbias"], "chain dbias")
    return y, gamma, beta, rel_is, bd["rho"].reshape(-1)


BN_SEEDS = {"plain": 2, "pool": 1, "shifted": 2}      # chosen on the CPU for the gate precondition


def test_bn_chain_plain(L):
    """reduce_stats -> colsum -> bn_fwd_finalize -> apply, then bwd_reduce -> colsum -> bn_bwd_finalize -> apply_bwd;
    N = 3, C = 48, 10 x 20; bounds: chain_bounds (the propagation is written out there)"""
    _bn_chain(L, BN_SEEDS["plain"], 10, 20, False)


def test_bn_chain_pool(L):
    """the same with MaxPool2d(2), on a 10 x 12 map"""
    _bn_chain(L, BN_SEEDS["pool"], 10, 12, True)


def test_bn_chain_shifted_mean(L):
    """|mean| / std = 16 per channel.  The batch variance is E[y^2] - mean^2 from fp32 partial sums, so its bound scales
    with E[y^2] / var = 257: loose by construction (chain_bounds).  Prints the measured relative error of invstd next
    to that of torch's fp32 CPU BatchNorm (DESIGN.md records both)."""
    y, gamma, beta, rel_is, rho = _bn_chain(L, BN_SEEDS["shifted"], 10, 20, False, shift_ratio=16.0)
    y64 = y.astype(np.float64)
    is_ref = 1 / np.sqrt(y64.var(axis=(0, 1, 2)) + EPS)
    yt = torch.from_numpy(np.ascontiguousarray(y.transpose(0, 3, 1, 2)))
    C = y.shape[-1]
    _, _, is32 = torch.native_batch_norm(yt, torch.ones(C), torch.zeros(C), None, None, True, 0.1, EPS)
    rel_t = np.abs(is32.numpy().astype(np.float64) - is_ref) / is_ref
    print(f"\nshifted mean (|mean|/std = 16): invstd relative error, max over channels: kernel chain "
          f"{rel_is.max():.3e}, torch fp32 CPU {rel_t.max():.3e}, ratio {rel_is.max() / rel_t.max():.2f}; "
          f"mean over channels: {rel_is.mean():.3e} vs {rel_t.mean():.3e}; derived bound {rho.max():.3e}")


GN_SEED = 1


def test_gn_chain_film(L):
    """reduce_stats -> gn_fwd_finalize -> apply (ReLU, FiLM), then bwd_reduce mode 2 -> slab_sum_nc rows 2 / 3,
    gn_bwd_finalize -> col_sum3 -> apply_bwd, against fp64 y = x + bias; GroupNorm(8, 48); ReLU; a u + b with the
    gradients of y, gamma, beta, bias, a, b.  Bounds: chain_bounds with per-(sample, group) statistics."""
    rng = np.random.default_rng(GN_SEED)
    N, C, G, H, W, csize = 3, 48, 8, 10, 20, 128
    q, HW = C // G, H * W
    bias = rng.standard_normal(C).astype(np.float32)
    y = ((rng.standard_normal((N, H, W, C)) * (0.5 + rng.random(C))).astype(np.float32) + bias).astype(np.float32)
    y64 = y.astype(np.float64)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    gamma = f32(1.0 + 0.5 * rng.standard_normal(C)); beta = f32(0.5 * rng.standard_normal(C))
    fa = f32(rng.standard_normal((N, C))); fb = f32(rng.standard_normal((N, C)))
    g = f32(rng.standard_normal((N, H, W, C)))
    xt = (_nchw(y64) - torch.from_numpy(bias.astype(np.float64)).reshape(1, C, 1, 1)).requires_grad_()
    bt = torch.from_numpy(bias.astype(np.float64)).requires_grad_()
    gn = torch.nn.GroupNorm(G, C, eps=EPS).double()
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(gamma)); gn.bias.copy_(torch.from_numpy(beta))
    at = torch.from_numpy(fa).requires_grad_(); btf = torch.from_numpy(fb).requires_grad_()
    yt = xt + bt.reshape(1, C, 1, 1)
    yt.retain_grad()
    o = at.reshape(N, C, 1, 1) * torch.relu(gn(yt)) + btf.reshape(N, C, 1, 1)
    o.backward(_nchw(g))
    yg = y64.reshape(N, HW, G, q)
    mu = yg.mean(axis=(1, 3)); var = yg.var(axis=(1, 3)); is_ref = 1 / np.sqrt(var + EPS)          # [N, G]
    s_ref = gamma[None] * np.repeat(is_ref, q, axis=1); t_ref = beta[None] - np.repeat(mu, q, axis=1) * s_ref
    assert _gate_ok(y64, bc(s_ref), bc(t_ref)), "seed precondition: a pre-activation within 1e-6 of the gate"
    gpre, _, _, _, _ = bwd_ref(2, g, y64, s_ref, t_ref, mu, is_ref, q, fa)
    k = n_add(C, csize) + 8
    r4 = lambda a: a.reshape(N, HW, G, q)   # noqa: E731
    bd = chain_bounds(yg, gamma.reshape(G, q), beta.reshape(G, q), k, k, r4(gpre), r4(g),
                      fa.reshape(N, 1, G, q), fb.reshape(N, 1, G, q))
    yd = T(y); nch = -(-HW // csize)
    slab = Z(N, nch, 2, C)
    L.cdm_reduce_stats(P(yd), C, N, HW, C, csize, P(slab), _s())
    mean, invstd, scale, shift = Z(N, G), Z(N, G), Z(N, C), Z(N, C)
    gd_, bd_, fad, fbd = T(gamma), T(beta), T(fa), T(fb)
    L.cdm_gn_fwd_finalize(P(slab), N, nch, 2, C, G, float(HW * q), P(gd_), P(bd_), EPS, P(mean), P(invstd), P(scale),
                          P(shift), _s())
    out = Z(N, H, W, C)
    L.cdm_norm_apply_fwd(2 | 8, P(yd), C, N, H, W, C, P(scale), P(shift), C, P(fad), C, P(fbd), C, None, None, None, N,
                         P(out), C, None, _s())
    rel_is = np.abs(Hh(invstd) - is_ref) / is_ref
    check(rel_is, 0 * rel_is, bd["rho"].reshape(N, G), "gn chain invstd (relative)")
    check(Hh(out), _nhwc(o), bd["dout"].reshape(N, H, W, C), "gn chain output")
    gdv = T(g)
    slab5 = Z(N, nch, 5, C)
    L.cdm_norm_bwd_reduce(2, P(gdv), C, P(yd), C, N, H, W, C, P(scale), P(shift), C, P(mean), P(invstd), G, q, P(fad), C,
                          csize, P(slab5), _s())
    da, db = Z(N, C), Z(N, C)
    L.cdm_slab_sum_nc(P(slab5), N, nch, 5, 2, C, P(da), _s())
    L.cdm_slab_sum_nc(P(slab5), N, nch, 5, 3, C, P(db), _s())
    co = [Z(N, C) for _ in range(6)]                                   # A B Cc pdg pdb pdbias
    L.cdm_gn_bwd_finalize(P(slab5), N, nch, C, G, float(HW * q), HW, P(gd_), P(invstd), *[P(v) for v in co], _s())
    dgamma, dbeta, dbias = Z(C), Z(C), Z(C)
    L.cdm_col_sum3(P(co[3]), P(dgamma), P(co[4]), P(dbeta), P(co[5]), P(dbias), N, C, _s())
    dy = Z(N, H, W, C)
    L.cdm_norm_apply_bwd(2, P(gdv), C, P(yd), C, N, H, W, C, P(scale), P(shift), C, P(mean), P(invstd), G, q, P(fad), C,
                         P(co[0]), P(co[1]), P(co[2]), C, P(dy), C, None, _s())
    check(Hh(dy), _nhwc(yt.grad), bd["ddy"].reshape(N, H, W, C), "gn chain dy")
    check(Hh(dgamma), gn.weight.grad.numpy(), bd["dgamma"], "gn chain dgamma")
    check(Hh(dbeta), gn.bias.grad.numpy(), bd["dbeta"], "gn chain dbeta")
    check(Hh(dbias), bt.grad.numpy(), bd["dbias"], "gn chain dbias")
    check(Hh(da), at.grad.numpy(), bd["dfa"].reshape(N, C), "gn chain d FiLM a")
    check(Hh(db), btf.grad.numpy(), bd["dfb"].reshape(N, C), "gn chain d FiLM b")
