"""The references of tests/_conv_ref.py against independent truth (torch's fp64 autograd), and the conditions under
which tests/test_gpu_halo_ops.py may ask for bit-equality, checked on the data of every one of its cases (no GPU): the
GPU tests cannot pass by sharing an error with their own reference, and their exactness claim rests on checked
arithmetic."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import test_gpu_halo_ops as G

LIMIT = 2.0 ** 24


def _close(a, b, what):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), what


def test_refs_match_autograd_of_conv_bn_relu_conv():
    """Conv2d -> BatchNorm2d (train) -> ReLU -> Conv2d in torch fp64: the forward and the three gradients equal
    bn_relu_stage / bn_bwd_stage plus the conv references, with the staging coefficients derived from the batch
    statistics the way the engine does (cdm_bn_fwd_finalize / cdm_bn_bwd_finalize): s = gamma invstd,
    t = beta - mean s, A = gamma invstd, B = -A S1 / n, Cc = -A S2 / n with S1 = sum g', S2 = sum g' xhat,
    g' = (y s + t > 0 ? g : 0), xhat = (y - mean) invstd."""
    rng = np.random.default_rng(3)
    N, H, C0, C1, C2, eps = 2, 6, 4, 6, 5, 1e-5
    x = rng.standard_normal((N, H, H, C0)); W1 = rng.standard_normal((C1, C0, 3, 3)); b1 = rng.standard_normal(C1)
    W2 = rng.standard_normal((C2, C1, 3, 3)); b2 = rng.standard_normal(C2)
    gamma = rng.standard_normal(C1); beta = rng.standard_normal(C1); r = rng.standard_normal((N, H, H, C2))
    t_ = {k: torch.from_numpy(v).requires_grad_() for k, v in dict(W1=W1, b1=b1, W2=W2, b2=b2, gamma=gamma,
                                                                   beta=beta).items()}
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_()
    yt = F.conv2d(xt, t_["W1"], t_["b1"], padding=1)
    zt = F.relu(F.batch_norm(yt, None, None, t_["gamma"], t_["beta"], training=True, eps=eps))
    ot = F.conv2d(zt, t_["W2"], t_["b2"], padding=1)
    (ot * torch.from_numpy(r).permute(0, 3, 1, 2)).sum().backward()

    y = R.conv3x3(x, W1, b1)
    _close(y, yt.detach().permute(0, 2, 3, 1).numpy(), "conv3x3")
    n = N * H * H
    mean = y.reshape(n, C1).mean(0); invstd = 1.0 / np.sqrt(y.reshape(n, C1).var(0) + eps)
    s = gamma * invstd; t = beta - mean * s
    z = R.bn_relu_stage(y, s, t)
    _close(R.conv3x3(z, W2, b2), ot.detach().permute(0, 2, 3, 1).numpy(), "bn_relu_stage + conv3x3")
    g = R.conv3x3_dgrad(r, W2)
    gp = np.where(y * s + t > 0, g, 0.0).reshape(n, C1); xh = ((y - mean) * invstd).reshape(n, C1)
    A = gamma * invstd; B = -A * gp.sum(0) / n; Cc = -A * (gp * xh).sum(0) / n
    dy = R.bn_bwd_stage(g, y, s, t, mean, invstd, A, B, Cc)
    _close(R.conv3x3_dgrad(dy, W1), xt.grad.permute(0, 2, 3, 1).numpy(), "bn_bwd_stage + conv3x3_dgrad")
    _close(R.conv3x3_wgrad(dy, x), t_["W1"].grad.numpy(), "bn_bwd_stage + conv3x3_wgrad")
    _close(R.conv3x3_wgrad(r, z), t_["W2"].grad.numpy(), "conv3x3_wgrad of the staged input")
    # the fp32-sequence forms are the same functions up to fp32 rounding
    assert np.abs(R.bn_bwd_stage(R.f32(g), R.f32(y), *[R.f32(v) for v in (s, t, mean, invstd, A, B, Cc)], f32ops=True)
                  - dy).max() <= 1e-5 * np.abs(dy).max()
    # sum|term| functions dominate the results
    assert (R.conv3x3_mag(x, W1, b1) >= np.abs(y) - 1e-12).all()


def test_epilogue_stats_keys_and_eval_forms():
    v = np.array([[-3.0, 1.0]]); old = np.array([[2.0, -4.0]]); b = np.array([0.5, 0.5])
    assert np.array_equal(R.epilogue(v, 0, None, b), [[-2.5, 1.5]])
    assert np.array_equal(R.epilogue(v, R.EPI_ACCUM, old, b), [[-0.5, -2.5]])
    assert np.array_equal(R.epilogue(v, R.EPI_RELU | R.EPI_ACCUM, old, b), [[0.0, 0.0]])      # relu after the add
    assert np.array_equal(R.epilogue(np.array([[-3.0, 3.0]]), 3, np.array([[4.0, -1.0]])), [[1.0, 2.0]])
    assert np.array_equal(R.epilogue(np.array([1.00390625]), 0, to_bf16=True), [1.0])        # 1 + 2^-8: ties to even
    assert np.array_equal(R.bf16(np.array([1.01171875, R.SENT])), [1.015625, 776.0])         # 1 + 3 2^-8 -> 1 + 2^-6
    rng = np.random.default_rng(0)
    y = rng.standard_normal((2, 16, 16, 3))
    s, q = R.tile_stats(y)
    assert s.shape == (4, 3) and np.allclose(s[1], y.reshape(-1, 3)[128:256].sum(0))
    assert np.allclose(q[3], (y.reshape(-1, 3)[384:] ** 2).sum(0))
    k = R.ymm_keys(y)
    f = np.array([-2.0, -1.0, -0.0, 0.0, 1e-40, 1.0, 3.0], dtype=np.float32)
    assert (np.diff(R.fkey(f).astype(np.int64)) >= 0).all() and R.fkey(np.float32(0.0)) == 0      # order-preserving
    assert np.array_equal(k[0], R.fkey(y.reshape(-1, 3).max(0))) and np.array_equal(k[1], R.fkey(y.reshape(-1, 3).min(0)))
    v = np.maximum(y, 0.0)
    pool = F.max_pool2d(torch.from_numpy(v).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.eval_fused(3, v), pool)
    sx = rng.standard_normal((2, 16, 16)); sw = rng.standard_normal((2, 3)); sb = rng.standard_normal((2, 3))
    out = R.eval_fused(1, v, sx, sw, sb, 1)
    assert np.allclose(out[0], sw[0] * sx[0][..., None] + sb[0] + v[0]) and np.allclose(out[1], sw[1] * sx[1][..., None]
                                                                                         + sb[1] + v[1])
    assert np.allclose(R.eval_fused(1, v, sx, sw, sb, 2)[1], sw[0] * sx[1][..., None] + sb[0] + v[1])
    fa = rng.standard_normal((2, 3)); fb = rng.standard_normal((2, 3))
    assert np.allclose(R.eval_fused(2, v, fa=fa, fb=fb)[1], fa[1] * v[1] + fb[1])
    assert np.allclose(R.eval_fused(2, v, fa=fa[:1], fb=fb[:1])[1], fa[0] * v[1] + fb[0])


def test_fma32_is_correctly_rounded():
    """fma32 against the exact rational a b + c rounded once to fp32, on random fp32 triples and on triples built so
    that the fp64 sum falls on or next to an fp32 tie (where rounding the fp64 sum again would go wrong)"""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    a, b = R.f32(rng.standard_normal(1500)), R.f32(rng.standard_normal(1500))
    c = R.f32(rng.standard_normal(1500) * 10.0 ** rng.integers(-6, 3, 1500))
    # a b = h (1 - 2^-46) with h half an fp32 ulp of c: a b + c lies 2^-70 |c| below a tie, which the fp64 sum cannot
    # hold (it rounds to the tie itself, and then to even: wrong whenever c is odd)
    c2 = R.f32(rng.standard_normal(500) * 4.0)
    a2 = np.full(500, 1.0 + 2.0 ** -23) * np.sign(c2)
    b2 = (1.0 - 2.0 ** -23) * 0.5 * R.ulp(c2)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])

    def rne32(q):   # the exact rational q rounded to nearest-even fp32
        lo = np.float32(float(q))                          # float(q) is correctly rounded to fp64; its fp32 image is
        cand = sorted({lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))},
                      key=lambda v: (abs(Fraction(float(v)) - q), int(np.float32(v).view(np.int32)) & 1))
        return float(cand[0])                              # within one fp32 step of the answer: choose among 3

    want = np.array([rne32(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    got = R.fma32(a, b, c)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} differ"
    naive = R.f32(a * b + c)
    assert (naive != want).any(), "no double-rounding case in the data: the test would not tell the two apart"


def test_unit_budget_and_fit_predicates():
    assert R.unit(np.array([0.375, -2.0, 0.0])) == 0.125 and R.unit(np.zeros(3)) == 1.0 and R.unit([3.0, 12.0]) == 1.0
    assert R.budget(np.array([6.0]), np.array([0.125]), np.array([0.25]), np.array([0.5])) == 6.0 * 32
    assert R.fits_bf16([1.0, 255.0, -0.0078125]) and not R.fits_bf16([257.0])
    assert R.fits_h3([1.0, 2047.0 / 2048.0], 1.0) and not R.fits_h3([1.0 + 2.0 ** -11], 1.0)
    assert R.h3_scale(1.0) == 2.0 ** 13 and R.h3_scale(0.75) == 2.0 ** 14


def _amax_bound(c):
    """cdm_bn_bwd_amax_bound on the CPU: max_c |A| max|g| + |B| + |Cc| (max|y| + |mean|) invstd"""
    s, t, mean, invstd, A, B, Cc = c["co"]
    return float((np.abs(A) * np.abs(c["g"]).max() + np.abs(B) + np.abs(Cc) * (np.abs(c["y"]).max() + np.abs(mean))
                  * invstd).max())


def _staged_ok(v, nterm, amax, what):
    assert R.fp32_exact(v), what
    assert R.fits16(v, nterm, amax), f"{what}: not representable in the 16-bit staging form of nterm {nterm}"


@pytest.mark.parametrize("case", G.FWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fwd_cases_are_exact(case):
    W, N, Cin, Cout, flags, bias, stats, data = case
    if data != "exact":
        return
    c = R.fwd_case(W, N, Cin, Cout, flags, bias, data, 0)
    for nterm in (4, 1):
        _staged_ok(c["x"], nterm, None, "x"); _staged_ok(c["Wt"], nterm, None, "W")
    assert R.budget(c["mag"], c["x"], c["Wt"], c["b"], c["old"]) < LIMIT
    assert R.fp32_exact(c["ref"]) and (c["b"] is None or ((c["b"] > 0).any() and (c["b"] < 0).any()))
    if flags == (R.EPI_RELU | R.EPI_ACCUM):   # the order of accumulate and relu is visible
        other = np.maximum(R.conv3x3(c["x"], c["Wt"], c["b"]), 0.0) + c["old"]
        assert (other != c["ref"]).any()


@pytest.mark.parametrize("case", G.PRE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pre_cases_are_exact(case):
    W, N, Cin, Cout, nterm, dt, data = case
    if data != "exact":
        return
    c = R.pre_case(W, N, Cin, Cout, dt, data, 0)
    assert np.array_equal(c["z_f32"], c["z_plain"]) and np.array_equal(c["z"], c["z_plain"])
    _staged_ok(c["z"], nterm, np.abs(c["z"]).max(), "z"); _staged_ok(c["Wt"], nterm, None, "W")
    assert dt & 1 == 0 or R.fits_bf16(c["x"])
    assert R.budget(c["mag"], c["z"], c["Wt"], c["b"]) < LIMIT
    assert (c["t"] > 0).any() and (c["t"] < 0).any() and set(np.abs(c["s"])) <= {0.5, 1.0, 2.0}
    # the shift applied to the zero padding would show: some border output changes
    zp = np.pad(c["x"], ((0, 0), (1, 1), (1, 1), (0, 0)))
    zp = np.maximum(zp * c["s"] + c["t"], 0.0)
    wrong = R._nhwc(F.conv2d(R._nchw(zp), R._t(c["Wt"]), R._t(c["b"])))
    assert (R.epilogue(wrong, 0, to_bf16=bool(dt & 2)) != c["ref"]).any()


@pytest.mark.parametrize("case", G.DGRAD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_dgrad_cases_are_exact(case):
    W, N, C, Cout, flags, want_amax, want_dy, nterm, dt, data = case
    if data == "gauss":
        return
    mode, ops = G.mode_of(data, nterm)
    c = R.dgrad_case(W, N, C, Cout, flags, dt, data, ops)
    s, t, mean, invstd, A, B, Cc = c["co"]
    assert np.array_equal(c["dy32"], c["dy_plain"]), "the fp32 sequence of bn_bwd_elem is not exact on this data"
    assert (B != 0).all() and (Cc * mean * invstd != 0).all() and (invstd > 0).all()
    assert _amax_bound(c) >= np.abs(c["dy32"]).max()
    assert dt & 1 == 0 or (R.fits_bf16(c["g"]) and R.fits_bf16(c["y"]))
    assert c["old"] is None or dt & 2 == 0 or R.fits_bf16(c["old"])
    _staged_ok(c["Wt"], nterm, None, "W")
    if mode == "exact":
        _staged_ok(c["dy"], nterm, _amax_bound(c), "dy")
        assert R.budget(c["mag"], c["dy"], c["Wt"], c["old"]) < LIMIT
    else:   # "fine", nterm 1: the bf16 rounding of dy must not be the identity
        assert not R.fits_bf16(c["dy32"])


@pytest.mark.parametrize("case", G.FUSED_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fused_cases_are_exact(case):
    kind, W, Cin, Cout, var, nterm, data = case
    if data != "exact":
        return
    c = R.fused_case(kind, W, Cin, Cout, var, data, 0)
    _staged_ok(c["x"], nterm, None, "x"); _staged_ok(c["Wt"], nterm, None, "W")
    assert R.budget(R.conv3x3_mag(c["x"], c["Wt"], c["b"]), c["x"], c["Wt"], c["b"]) < LIMIT
    # the transform: one fma of exact operands plus (kind 1) one add; exact when its results are fp32 values
    assert R.fp32_exact(c["ref"]) and R.fp32_exact(c["v"])
    if kind == 1:
        sel = (np.arange(3) >= var).astype(int)
        assert R.fp32_exact(c["sc_w"][sel][:, None, None, :] * c["sc_x"][..., None] + c["sc_b"][sel][:, None, None, :])


def _wgrad_sp(case):
    Cin, Cout, W, N, eng = case[:5]
    return R.engine_wgrad_splits(N * W * W, Cout, Cin) if eng else 1


def test_wgrad_dispatch_restated():
    """effective_splits / wgrad_ks on values worked by hand from csrc/conv_wgrad.hip"""
    assert R.effective_splits(1024, 64) == 64 and R.effective_splits(1024, 64, 32) == 32     # 64 / 32 steps
    assert R.effective_splits(12288, 256) == 256 and R.effective_splits(12288, 256, 32) == 192
    assert R.effective_splits(100, 7) == 7 and R.effective_splits(16, 5) == 1 and R.effective_splits(4096, 0) == 1
    assert R.engine_wgrad_splits(8192, 128, 256) == 128 and R.engine_wgrad_splits(256, 128, 128) == 16
    assert R.wgrad_ks(1, 64, 1, 4, 0) == 4 and R.wgrad_ks(1, 64, 1, 1, 0) == 2 and R.wgrad_ks(1, 64, 1, 1, 2) == 4
    assert R.wgrad_ks(1, 48, 1, 4, 0) == 1 and R.wgrad_ks(1, 32, 64, 4, 0) == 1 and R.wgrad_ks(2, 64, 128, 4, 0) == 4
    assert R.wgrad_ks(1, 64, 128, 4, 0) == 2           # 128 splits of 64 64-pixel steps: h3 falls back to 32 pixels


def test_wgrad_cases_cover_the_dispatch():
    """what section (e) is for, counted from the case lists with the launcher's rules: every (dY, X, arithmetic)
    staging triple on exact data; every K step in both arithmetics, with both transforms staged, on exact data, with
    one split and with several; bf16 operands of every kind; every shape and width of the list"""
    ex = [c for c in G.WGRAD_CASES if c[9] == "exact"]
    assert {(bn, px, nt) for _, _, _, _, _, bn, px, nt, _, _, _ in ex} == {(b, p, n) for b in (False, True)
                                                                          for p in (False, True) for n in (4, 1)}
    both = {(c[7], c[10], _wgrad_sp(c) > 1) for c in ex if c[5] and c[6]}
    assert both >= {(nt, ks, True) for nt in (4, 1) for ks in (1, 2, 4)}
    assert both >= {(nt, ks, False) for nt in (4, 1) for ks in (2, 4)}       # one split: the steps that need W % 32 == 0
    assert {c[8] for c in ex} == {0, 1, 2, 3}
    assert {(c[0], c[1]) for c in ex} == {(128, 128), (256, 128), (128, 256)} and {c[2] for c in ex} == {16, 32, 48, 64}
    assert {c[3] for c in ex} >= {1, 3} and {c[4] for c in ex} == {False, True}
    assert {c[10] for c in G.SUMS_CASES} == {1, 2, 4}


@pytest.mark.parametrize("case", G.WGRAD_CASES + G.SUMS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_wgrad_cases_are_exact(case):
    Cin, Cout, W, N, eng, bn, px, nterm, dt, data, ks = case
    assert R.wgrad_ks(N, W, _wgrad_sp(case), nterm, dt) == ks, "the case does not run the K step it names"
    if data == "gauss":
        return
    mode, ops = G.mode_of(data, nterm)
    c = R.wgrad_case(Cin, Cout, W, N, bn, px, data, 0)
    assert N * W * W <= 12288
    assert np.array_equal(c["dy"], c["dy_plain"]) and np.array_equal(c["X"], c["X_plain"])
    assert dt & 1 == 0 or (R.fits_bf16(c["g"]) and R.fits_bf16(c["y"]))
    assert dt & 2 == 0 or R.fits_bf16(c["x"])
    assert (c["xt"] > 0).any() and (c["xt"] < 0).any() and len(set(c["xt"])) > 4
    _staged_ok(c["X"], nterm, np.abs(c["X"]).max(), "X")
    if mode == "exact":
        _staged_ok(c["dy"], nterm, np.abs(c["dy"]).max(), "dY")
        assert R.budget(c["mag"], c["dy"], c["X"]) < LIMIT
    else:
        assert not R.fits_bf16(c["dy"])
