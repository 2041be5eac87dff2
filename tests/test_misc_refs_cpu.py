"""The references of tests/_misc_ref.py against independent truth (torch's fp64 operators and autograd), the exactness
the dyadic generators claim, and the derived bounds (no GPU): the GPU tests of csrc/misc.hip cannot pass by sharing an
error with their own reference."""
import math

import numpy as np
import pytest
import torch

import _misc_ref as M


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _ok_bound(b, some=False):
    """finite and non-zero; some=True: non-zero somewhere (a tap that only meets padding has the exact sum 0)"""
    b = np.asarray(b, dtype=np.float64)
    return bool(np.all(np.isfinite(b)) and (b.max() > 0 if some else np.all(b > 0)))


def test_gelu_matches_torch():
    x = np.linspace(-9.0, 9.0, 3601)
    xt = torch.from_numpy(x).requires_grad_()
    g = torch.nn.GELU()(xt)
    g.sum().backward()
    assert (np.abs(M.gelu(x) - g.detach().numpy()) <= 4 * 2.0 ** -52 * (1 + np.abs(x))).all()
    gp, err = M.gelu_grad(x)
    assert (np.abs(gp - xt.grad.numpy()) <= 4 * 2.0 ** -52 * (1 + np.abs(x))).all()
    assert _ok_bound(err)


@pytest.mark.parametrize("rows,in_dim,E", M.MLPS_A + [M.MLP_B])
def test_embed_stages_match_autograd(rows, in_dim, E):
    """the staged references (each stage fed the previous one's exact output) against Linear -> GELU -> Linear"""
    d = M.embed_inputs(np.random.default_rng(E + rows), rows, in_dim, E)
    t = {k: torch.from_numpy(v).requires_grad_() for k, v in d.items() if k != "dout"}
    out = torch.nn.functional.linear(torch.nn.GELU()(torch.nn.functional.linear(t["x"], t["w1"], t["b1"])), t["w2"],
                                     t["b2"])
    out.backward(torch.from_numpy(d["dout"]))
    pre, h, o, mag = M.embed_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
    assert _rel(o, out.detach().numpy()) <= 1e-12
    dpre, bound = M.embed_dpre(d["dout"], d["w2"], pre)
    g = M.embed_param_grads(d["dout"], h, dpre, d["x"])
    for k, name in (("w2", "dw2"), ("b2", "db2"), ("w1", "dw1"), ("b1", "db1")):
        assert _rel(g[name][0], t[k].grad.numpy()) <= 1e-12, name
        assert _ok_bound(M.sum_bound(*g[name])), name
    dx, dxb = M.embed_input_grad(dpre, d["w1"])
    assert _rel(dx, t["x"].grad.numpy()) <= 1e-12
    assert _ok_bound(bound) and _ok_bound(dxb) and _ok_bound(M.sum_bound(o, mag))
    # the two-input form is the sum of two one-input forms
    dx2, dx2b = M.embed_input_grad(dpre, d["w1"], 2 * dpre, d["w1"])
    assert _rel(dx2, 3 * dx) <= 1e-12 and _ok_bound(dx2b)


@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES)
def test_cin1_refs_match_torch(N, H, W, C):
    rng = np.random.default_rng(H * W + C)
    x = M.gauss(rng, (N, H, W)); w9 = M.gauss(rng, (9, C)); b = M.gauss(rng, C); dy = M.gauss(rng, (N, H, W, C))
    y, xt, wt, bt = M.torch_cin1(x, w9, b)
    y.backward(torch.from_numpy(dy))
    got, mag = M.cin1_fwd(x, w9, b, 0)
    assert _rel(got, y.detach().numpy()) <= 1e-12 and _ok_bound(M.chain_bound(3, mag))
    assert _rel(M.cin1_fwd(x, w9, b, 1)[0], np.maximum(y.detach().numpy(), 0)) <= 1e-12
    terms = M.cin1_wgrad_terms(dy, x)
    dw = wt.grad.numpy().reshape(C, 9).T
    for csize in (128, 50, H * W + 3):
        part = M.chunk_sums(terms, csize)                                   # [N, nch, 10, C]
        assert part.shape[1] == -(-(H * W) // csize)
        tot = part.sum(axis=(0, 1))
        assert _rel(tot[:9], dw) <= 1e-12 and _rel(tot[9], bt.grad.numpy()) <= 1e-12
        assert _ok_bound(M.chain_bound(M.lanes_n(C, min(csize, H * W)), M.chunk_sums(np.abs(terms), csize)), some=True)


@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES)
def test_cout1_refs_match_torch(N, H, W, C):
    rng = np.random.default_rng(H * W + C + 1)
    z = M.gauss(rng, (N, H, W, C)); w = M.gauss(rng, (C, 9)); b = 0.375; deps = M.gauss(rng, (N, H, W))
    out, zt, wt = M.torch_cout1(z, w, b)
    out.backward(torch.from_numpy(deps))
    got, mag = M.cout1_fwd(z, w, b)
    assert _rel(got, out.detach().numpy()) <= 1e-12 and _ok_bound(mag)
    dz, dmag = M.cout1_dgrad(deps, w)
    assert _rel(dz, zt.grad.numpy().transpose(0, 2, 3, 1)) <= 1e-12 and np.all(np.isfinite(dmag))
    dw = wt.grad.numpy().reshape(C, 9).T                                    # [9][C]
    ct = M.cout1_wgrad_chunk_terms(deps, z)
    for csize in (128, 50):
        assert _rel(M.chunk_sums(ct, csize).sum(axis=(0, 1)), dw) <= 1e-12
    bt = M.cout1_wgrad_band_terms(deps, z)
    for R in sorted({1, 2, H}):
        if H % R:
            continue
        part = M.band_sums(bt, W, R)
        assert part.shape == (N * H // R, 9, C)
        assert _rel(part.sum(axis=0), dw) <= 1e-12
    # a band's partial is not the chunk partial of the same pixels (the two forms split the sum differently)
    if H > 1 and W > 1:
        assert not np.allclose(M.band_sums(bt, W, 1), M.band_sums(ct, W, 1))


def test_cout1_gn_refs_match_torch():
    N, H, W, C = 2, 4, 8, 16
    rng = np.random.default_rng(9)
    y = M.gauss(rng, (N, H, W, C)); gs = M.gauss(rng, (N, C)); gt = M.gauss(rng, (N, C)); w = M.gauss(rng, (C, 9))
    deps = M.gauss(rng, (N, H, W))
    z = np.maximum(y * gs[:, None, None, :] + gt[:, None, None, :], 0.0)
    out, _, wt = M.torch_cout1(z, w, 0.25)
    out.backward(torch.from_numpy(deps))
    assert _rel(M.cout1_fwd(y, w, 0.25, gs, gt)[0], out.detach().numpy()) <= 1e-12
    part = M.band_sums(M.cout1_wgrad_band_terms(deps, y, gs, gt), W, 2)
    assert _rel(part.sum(axis=0), wt.grad.numpy().reshape(C, 9).T) <= 1e-12


def test_shift_is_zero_padded():
    a = np.arange(1.0, 13.0).reshape(1, 3, 4)
    assert np.array_equal(M.shift(a, 0, 0), a)
    assert np.array_equal(M.shift(a, 1, 0)[0], np.vstack([a[0, 1:], np.zeros((1, 4))]))
    assert np.array_equal(M.shift(a, 0, -1)[0], np.hstack([np.zeros((3, 1)), a[0, :, :-1]]))
    assert not M.shift(np.ones((1, 1, 1)), 1, 1).any()


# ----------------------------------------------------------------------------------------------------------------
# the exactness the dyadic generators claim
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4099, 65536])
def test_mse_dyadic_sums_are_exact(n):
    rng = np.random.default_rng(n)
    pred, noise = M.mse_inputs(rng, n)
    d = pred - noise
    assert M.sums_exact_in_fp32((d * d)[None]) and M.grid_units((d * d)[None], 2.0 ** -6) <= 2 ** 24
    for gn in (n, 1.5 * n):
        scale = float(np.float32(2.0 / gn))
        g = (d.astype(np.float32) * np.float32(scale)).astype(np.float64)
        if math.log2(gn).is_integer():
            assert np.array_equal(g, d * 2.0 / gn) and M.sums_exact_in_fp32(g[None])
    # worst case of the claim: every |d| = 2
    worst = np.full((1, 65536), 4.0)
    assert M.sums_exact_in_fp32(worst) and M.grid_units(worst, 2.0 ** -6) == 2 ** 24
    for nb in (1, 3, 64):
        bs = M.mse_block_sums(d * d, n, nb)
        assert bs.sum() == (d * d).sum() and (bs[-(-n // 256):] == 0).all()
        assert _ok_bound(M.mse_dbias_k(n, nb) * M.U * (np.abs(d).sum() + 1.0))


@pytest.mark.parametrize("HW", [1, 100, 256, 257, 1000])
def test_mse_accum_dyadic_sums_are_exact(HW):
    rng = np.random.default_rng(HW)
    pred, noise = M.mse_inputs(rng, 3 * HW)
    d = (pred - noise).reshape(3, HW)
    assert M.sums_exact_in_fp32(d * d)
    mul = np.array([2.0, 0.5, 4.0]); div = np.array([8.0, 2.0, 0.25]); acc0 = M.dyad(rng, 3)
    got = M.mse_accum32(acc0, pred, noise, HW, mul, div)
    ref = acc0 + (d * d).sum(axis=1) / HW * mul / div
    M.check(got, ref, 2 * M.ulp(ref), "fp32 sequence against fp64")      # one rounding of / HW, one of the +=
    assert M.mse_accum_k(HW) >= 18


@pytest.mark.parametrize("N,H,W,C", M.CONV_SHAPES)
def test_conv_dyadic_sums_are_exact(N, H, W, C):
    """the conv generator (multiples of 2^-4 in [-2, 2]): products are multiples of 2^-8 of at most 1024 units; a
    forward output adds 9 of them and a bias (16 x 32 units), a weight-gradient partial at most H W <= 900"""
    rng = np.random.default_rng(C + W)
    x = M.conv_dyad(rng, (N, H, W)); w9 = M.conv_dyad(rng, (9, C)); b = M.conv_dyad(rng, C)
    dy = M.conv_dyad(rng, (N, H, W, C)); w = M.conv_dyad(rng, (C, 9))
    step = M.GRID * M.GRID
    y, mag = M.cin1_fwd(x, w9, b, 0)
    assert mag.max() / step <= 2 ** 24 and np.array_equal(y, M.f32(y))
    dz, dmag = M.cout1_dgrad(x, w)
    assert dmag.max() / step <= 2 ** 24 and np.array_equal(dz, M.f32(dz))
    for terms in (M.cin1_wgrad_terms(dy, x), M.cout1_wgrad_chunk_terms(x, dy), M.cout1_wgrad_band_terms(x, dy)):
        assert M.sums_exact_in_fp32(terms)                                 # the whole image in one chunk / band
        assert M.grid_units(terms, step) <= 2 ** 24
    assert H * W * 1024 <= 2 ** 24


def test_bounds_vocabulary():
    assert M.lanes_n(4, 128) == 1 + 256 and M.lanes_n(1024, 50) == 50 + 1 and M.lanes_n(48, 128) == 7 + 21
    assert M.chain_bound(0, 1.0) == 8 * M.U
    assert M.sum_bound(1.0, 0.0) == 2.0 ** -23 and M.ulp(0.75) == 2.0 ** -24
    a = np.arange(20.0).reshape(1, 10, 2)
    assert np.array_equal(M.chunk_sums(a, 4)[0, :, 0], [0 + 2 + 4 + 6, 8 + 10 + 12 + 14, 16 + 18])
    assert np.array_equal(M.widen(np.ones((2, 3)), 5, 1), [[M.SENT, 1, 1, 1, M.SENT]] * 2)
    x = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(M.perturb32(x, x, np.array([0.5, 2.0]), np.array([0.25, 1.0])), [[0.75, 1.5], [9.0, 12.0]])
