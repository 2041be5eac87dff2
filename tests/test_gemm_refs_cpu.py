"""The references of tests/_gemm_ref.py against independent truth (torch's fp64 operators and autograd), and, on the data
of every exact case of tests/test_gpu_gemm_ops.py (no GPU): the conditions under which bit-equality is the right bar,
the launchers' dispatch predicates restated (every case lands on the path its comment names, with the block counts
that reach the XCD remap's remainder branch), and the sensitivity of the data: a deliberately wrong numpy emulation of
each error class the cases are about must be caught by `exact` on at least one listed case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R
from _gemm_ref import EPI_ACCUM, EPI_RELU, NT_H3, exact

LIMIT = 2.0 ** 24
ARITH = (NT_H3, 1)


def _close(a, b, what):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), what


def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------
# references against torch
# ----------------------------------------------------------------------------------------------------------------
def test_convT_refs_match_torch_autograd():
    rng = np.random.default_rng(1)
    N, H, W, Ci, Co = 3, 5, 7, 6, 4
    x, Wt, b = rng.standard_normal((N, H, W, Ci)), rng.standard_normal((Ci, Co, 2, 2)), rng.standard_normal(Co)
    dy = rng.standard_normal((N, 2 * H, 2 * W, Co))
    y, dx, dW = R.torch_convT(x, Wt, b, dy)
    _close(R.convT_fwd(x, Wt, b), y, "convT_fwd")
    _close(R.convT_dgrad(dy, Wt), dx, "convT_dgrad")
    _close(R.convT_wgrad(x, dy), dW, "convT_wgrad")
    for splits in (1, 2, 5):
        parts = R.convT_wgrad_parts(x, dy, splits)
        assert parts.shape[0] == R.effective_splits(N * H * W, splits)
        _close(parts.sum(0).reshape(Ci, 2, 2, Co).transpose(0, 3, 1, 2), dW, "convT_wgrad_parts")
    # the GEMM + scatter form, and the packed weights the kernels read
    _close(x.reshape(-1, Ci) @ R.convT_pack(Wt), R._convT_cols(R.convT_fwd(x, Wt)), "convT_pack")


def test_conv3x3_wgrad_parts_match_torch():
    rng = np.random.default_rng(2)
    N, H, W, Ci, Co = 2, 5, 8, 3, 4
    x, gy = rng.standard_normal((N, H, W, Ci)), rng.standard_normal((N, H, W, Co))
    ref = R.conv3x3_wgrad(gy, x)
    for splits in (1, 7):
        parts = R.conv3x3_wgrad_parts(gy, x, splits)
        assert parts.shape[0] == R.effective_splits(N * H * W, splits)
        _close(R.slab_to_oihw(parts.sum(0), Ci), ref, "conv3x3_wgrad_parts")
    y = rng.standard_normal((192, 3))
    s, q = R.tile_stats(y)
    assert s.shape == (2, 3) and np.allclose(s[1], y[128:].sum(0)) and np.allclose(q[1], (y[128:] ** 2).sum(0))


def test_gemm_refs_match_torch():
    rng = np.random.default_rng(3)
    M, K, N = 5, 37, 12
    a, b, bias, old = (rng.standard_normal(s) for s in ((M, K), (K, N), N, (M, N)))
    t = lambda v: torch.from_numpy(v)    # noqa: E731
    _close(R.gemm(a, b), torch.matmul(t(a), t(b)).numpy(), "gemm")
    _close(R.gemm(a, b, bias, 4), (t(a) @ t(b) + t(bias[:4]).repeat(3)).numpy(), "gemm bias_mod")
    _close(R.gemm(a, b, bias, N, EPI_RELU | EPI_ACCUM, old), F.relu(t(a) @ t(b) + t(bias) + t(old)).numpy(), "flags")
    at = rng.standard_normal((K, M))
    for splits in (1, 3):
        _close(R.gemm_parts(a, b, splits).sum(0), (t(a) @ t(b)).numpy(), "gemm_parts")
        _close(R.gemm_tn_parts(at, b, splits).sum(0), (t(at).T @ t(b)).numpy(), "gemm_tn_parts")
    assert R.split_ranges(272, 16) == [(32 * z, min(272, 32 * z + 32)) for z in range(9)]
    assert R.split_ranges(144, 4) == [(0, 48), (48, 96), (96, 144)] and R.split_ranges(5, 1) == [(0, 5)]


def test_slab_reduce_ref():
    rng = np.random.default_rng(4)
    Co, Ci, sp = 3, 2, 4
    slab = rng.standard_normal((sp, Co, 9 * Ci))                 # [z][co][tap Ci + ci]
    old = rng.standard_normal(Co * Ci * 9)
    got = R.slab_reduce(slab, old, 9 * Ci, 1, 9, Ci, 0, 1.0).reshape(Co, Ci, 3, 3)
    _close(got, R.slab_to_oihw(slab.sum(0), Ci), "OIHW repack")
    got = R.slab_reduce(slab, old, 9 * Ci, 0, 1, 0, 1, -2.0)
    _close(got, old - 2.0 * slab.sum(0).reshape(-1), "accumulate, scale, csplit 0")
    wide = R.slab_reduce(slab, np.full(Co * (9 * Ci + 4), R.SENT), 9 * Ci + 4, 0, 1, 9 * Ci, 0, 0.5)
    wide = wide.reshape(Co, -1)
    _close(wide[:, :9 * Ci], 0.5 * slab.sum(0), "s_m > N")
    assert (wide[:, 9 * Ci:] == R.SENT).all()


# ----------------------------------------------------------------------------------------------------------------
# exactness conditions of every exact case
# ----------------------------------------------------------------------------------------------------------------
def _fits(*ops):
    for a in ops:
        for nt in ARITH:
            assert R.fits16(a, nt), "an operand is not its own 16-bit image"
        assert np.abs(a).max() == 1.0, "max|operand| != 1: the h3 scale is not the known one"
        assert (a > 0).any() and (a < 0).any()


def _exact32(*arrays):
    for a in arrays:
        assert R.fp32_exact(a), "a reference value is not an fp32 number"


@pytest.mark.parametrize("case", R.FWD_CASES + R.DGRAD_CASES, ids=lambda c: c[0])
def test_exactness_convT_fwd_dgrad(case):
    c = R.convT_case(case[1], "exact", 0)
    _fits(c["x"], c["Wt"], c["b"], c["dy"], c["old"])
    assert R.budget(c["y_mag"] + np.abs(c["b"]), c["x"], c["Wt"], c["b"]) < LIMIT
    assert R.budget(c["dx_mag"] + np.abs(c["old"]), c["dy"], c["Wt"], c["old"]) < LIMIT
    _exact32(c["y"], c["y"] + c["b"], c["dx"], *[R.epilogue(c["dx"], f, c["old"]) for f in R.DGRAD_FLAGS])


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: c[0])
def test_exactness_convT_wgrad(case):
    c = R.convT_case(case[1], "exact", 0)
    _fits(c["x"], c["dy"])
    assert R.budget(R.convT_wgrad(np.abs(c["x"]), np.abs(c["dy"])), c["x"], c["dy"]) < LIMIT
    for splits in case[2]:
        _exact32(R.convT_wgrad_parts(c["x"], c["dy"], splits))
    _exact32(R.convT_wgrad(c["x"], c["dy"]))


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c[0])
def test_exactness_conv3x3(case):
    name, shape, kcs, flags, bias, stats = case
    c = R.conv_case(shape, "exact", 0)
    _fits(c["x"], c["Wt"], c["b"], c["gy"], c["old"])
    assert R.budget(c["y_mag"] + np.abs(c["b"]) + np.abs(c["old"]), c["x"], c["Wt"], c["b"], c["old"]) < LIMIT
    assert R.budget(c["dx_mag"], c["gy"], c["Wt"]) < LIMIT
    y = R.epilogue(c["y"], flags, c["old"], c["b"] if bias else None)
    _exact32(y, c["dx"])
    if stats:
        s, _ = R.tile_stats(y)
        sm, _ = R.tile_stats(np.abs(y))
        _exact32(s)
        assert R.budget(sm, y, np.ones(1)) < LIMIT, "a per-tile column sum is not exact in fp32"
    absw = R.conv3x3_wgrad_parts(np.abs(c["gy"]), np.abs(c["x"]), 1)
    assert R.budget(absw, c["gy"], c["x"]) < LIMIT
    for splits in R.CONV_WGRAD_SPLITS:
        _exact32(R.conv3x3_wgrad_parts(c["gy"], c["x"], splits))


@pytest.mark.parametrize("case", R.GEMM_CASES + R.TN_CASES, ids=lambda c: c[0])
def test_exactness_gemm(case):
    tn = case[0].startswith("TN")
    c = R.gemm_case(case[1], "exact", int(tn))
    a = c["a"].T if tn else c["a"]
    _fits(c["a"], c["b"], c["bias"], c["old"])
    mag = np.abs(a) @ np.abs(c["b"]) + np.abs(c["bias"]) + np.abs(c["old"])
    assert R.budget(mag, c["a"], c["b"], c["bias"], c["old"]) < LIMIT
    _exact32(R.gemm_tn_parts(c["a"], c["b"], case[2]) if tn else R.gemm_parts(c["a"], c["b"], case[2]))
    if not tn:
        for bias_mod, flags in case[3]:
            _exact32(R.gemm(a, c["b"], c["bias"] if bias_mod else None, max(bias_mod, 1), flags, c["old"]))


@pytest.mark.parametrize("M,N", R.REDUCE_SHAPES)
def test_exactness_slab_reduce(M, N):
    for splits in R.REDUCE_SPLITS:
        c = R.reduce_case(M, N, splits, "exact")
        # slab entries and old values are multiples of 2^-3, scale a power of two down to 2^-1: units of 2^-4
        assert np.array_equal(c["slab"] * 8, np.round(c["slab"] * 8)) and np.abs(c["slab"]).max() <= 1.0
        assert (np.abs(c["slab"]).sum(0).max() * 2.0 + 1.0) * 16 < LIMIT
        for scale in R.SCALES:
            for name, s_m, s_hi, s_lo, cs, size in R.reduce_perms(M, N):
                _exact32(R.slab_reduce(c["slab"], c["old"][:size], s_m, s_hi, s_lo, cs, 1, scale))
    names = {p[0] for p in R.reduce_perms(M, N)}
    assert {"identity", "csplit0", "wide"} <= names and names & {"oihw", "convT", "up0"}


def test_reduce_perm_coverage():
    """every permutation kind occurs, both kernels run at every shape but N = 6, and the float4 kernel's last block is
    partly empty at (5, 36) and (3, 8)"""
    kinds = set()
    for M, N in R.REDUCE_SHAPES:
        kinds |= {p[0] for p in R.reduce_perms(M, N)}
        on4 = {R.reduce4(N, s) for s in R.REDUCE_SPLITS}
        assert on4 == ({False} if N == 6 else {False, True})
    assert kinds == {"identity", "csplit0", "wide", "oihw", "convT", "up0"}
    assert [R.reduce4(8, s) for s in (7, 8)] == [False, True]
    for M, N in ((5, 36), (3, 8)):
        assert (M * N // 4) % 32 != 0


# ----------------------------------------------------------------------------------------------------------------
# dispatch predicates and block counts
# ----------------------------------------------------------------------------------------------------------------
def test_dispatch_convT_fwd():
    want = {"F0": (False, None), "F1": (False, None), "F2": (True, (3, 1)), "F3": (True, (2, 3)),
            "F4": (True, (11, 1)), "F5": (True, (1, 1))}
    for name, shape, dld, off in R.FWD_CASES:
        deep = R.deep_fwd(shape, shape[3] + dld)
        assert (deep, R.deep_grid(shape) if deep else None) == want[name], name
    assert R.xcd_qr(3) == (0, 3) and R.xcd_qr(6) == (0, 6) and R.xcd_qr(11) == (1, 3)
    fast = {c[0]: R.convT_fast_tiles(c[1]) for c in R.FWD_CASES}
    assert not any(fast["F0"].values()) and len(fast["F0"]) == 1                       # carry walk, partial tile
    assert {True, False} == set(fast["F1"].values()) and fast["F1"][0, 0] and not fast["F1"][64, 0] \
        and not fast["F1"][0, 128]                                                     # one block, both write-outs
    assert all(fast["F2"].values()) and R.FWD_CASES[2][1][1] != R.FWD_CASES[2][1][2]   # fast at W = 32, H != W
    assert all(fast["F3"].values()) and R.FWD_CASES[3][1][2] == 16                     # the W = 16 second-row offset
    assert all(fast["F4"].values())
    assert not any(fast["F5"].values()) and len(fast["F5"]) == 4                       # carry walk in full tiles
    assert R.FWD_CASES[1][1][3] % 16 == 4 and R.FWD_CASES[0][1][3] == 16               # K tail; one K tile
    assert R.FWD_CASES[5][2:] == (8, 4)


def test_dispatch_convT_dgrad():
    want = {"D0": None, "D1": (3, 1), "D2": (1, 2), "D3": None, "D4": (11, 1)}
    for name, shape, dld, off in R.DGRAD_CASES:
        deep = R.deep_dgrad(shape, shape[4] + dld)
        assert (R.deep_grid(shape, True) if deep else None) == want[name], name
    Co = R.DGRAD_CASES[2][1][4]
    # D2: the sub-pixel boundaries (K tiles 3, 6, 9) fall inside the unrolled loop's tile pairs (2t, 2t + 1) or between
    # them: both kinds occur
    b = [ij * Co // 16 for ij in (1, 2, 3)]
    assert b == [3, 6, 9] and {t % 2 for t in b} == {0, 1}
    Co3 = R.DGRAD_CASES[3][1][4]
    assert Co3 % 16 and any((ij * Co3) % 16 for ij in (1, 2, 3)) and R.DGRAD_CASES[3][1][3] % 128 == 4


def test_dispatch_convT_wgrad():
    want = {"W0": (False, None), "W1": (True, [4, 8]), "W2": (True, [12, 20]), "W3": (True, [24]), "W4": (False, None)}
    for name, shape, splits in R.WGRAD_CASES:
        tr = R.tr_wgrad(shape, shape[3] + 4, shape[4] + 4)
        assert (tr, [R.tr_grid(shape, s) for s in splits] if tr else None) == want[name], name
    K = 3 * 3 * 16
    assert R.split_ranges(K, 4) == [(0, 48), (48, 96), (96, 144)] and R.xcd_qr(12) == (1, 4)
    assert R.split_ranges(K, 5)[-1] == (128, 144) and len(R.split_ranges(K, 5)) == 5
    assert R.split_ranges(128, 3) == [(0, 48), (48, 96), (96, 128)]                   # W3: last split short
    # W2: a split's pixel range crosses an image seam (48 pixels per image, 48-pixel splits start on seams; the
    # 32-pixel splits of the 5-split run do not)
    assert any(k0 % 48 and k0 // 48 != (k1 - 1) // 48 for k0, k1 in R.split_ranges(K, 5))


def test_dispatch_conv3x3_and_gemm():
    inst = {c[0]: (R.conv_inst(c[1]), -(-c[1][0] * c[1][1] * c[1][2] // 128)) for c in R.CONV_CASES}
    assert inst == {"C0": ("generic", 1), "C1": ("generic", 2), "C2": ("128", 1), "C3": ("128-64", 64),
                    "C4": ("generic", 5), "C5": ("128", 11)}
    assert R.xcd_qr(5)[1] and R.xcd_qr(11)[1] and R.xcd_qr(64) == (8, 0)
    assert len(R.split_ranges(272, 16)) == 9 and R.split_ranges(272, 16)[-1] == (256, 272)
    assert R.split_ranges(40, 3) == [(0, 16), (16, 32), (32, 40)]


# ----------------------------------------------------------------------------------------------------------------
# sensitivity: each wrong emulation is caught on at least one listed case
# ----------------------------------------------------------------------------------------------------------------
def _fwd(case):
    c = R.convT_case(case[1], "exact", 0)
    return c, c["y"] + c["b"]


def test_sensitivity_convT_forward_errors():
    hit = {"subpixel": 0, "ktile": 0, "seam": 0, "row16": 0}
    for case in R.FWD_CASES:
        c, ref = _fwd(case)
        x, Wt, b = c["x"], c["Wt"], c["b"]
        hit["subpixel"] += _caught(lambda: exact(R.convT_fwd(x, Wt.transpose(0, 1, 3, 2), b), ref, "swap"))
        kt = (x.shape[-1] - 1) // 16 * 16                           # the last K tile dropped
        if kt:
            hit["ktile"] += _caught(lambda: exact(R.convT_fwd(x[..., :kt], Wt[:kt], b), ref, "ktile"))
        hit["seam"] += _caught(lambda: exact(R.convT_fwd_scatter(x, Wt, b, "seam"), ref, "seam"))
        if case[1][2] == 32:
            hit["row16"] += _caught(lambda: exact(R.convT_fwd_scatter(x, Wt, b, "row16"), ref, "row16"))
        elif case[1][2] == 16 and (case[1][1] * 16) % 32 == 0:
            exact(R.convT_fwd_scatter(x, Wt, b, "row16"), ref, "the W = 16 offset is right at W = 16")
    assert all(hit.values()), hit
    # the same sub-pixel swap and tile drop in the input gradient
    for case in R.DGRAD_CASES:
        c = R.convT_case(case[1], "exact", 0)
        assert _caught(lambda: exact(R.convT_dgrad(c["dy"], c["Wt"].transpose(0, 1, 3, 2)), c["dx"], "swap"))


def test_sensitivity_split_ranges():
    hit = 0
    for name, shape, splits in R.WGRAD_CASES:
        c = R.convT_case(shape, "exact", 0)
        for s in splits:
            ref = R.convT_wgrad_parts(c["x"], c["dy"], s)
            if ref.shape[0] > 1:
                hit += _caught(lambda: exact(R.convT_wgrad_parts(c["x"], c["dy"], s, shift=1), ref, "shift"))
        dW = R.convT_wgrad(c["x"], c["dy"])
        assert _caught(lambda: exact(dW.transpose(0, 1, 3, 2), dW, "sub-pixel swap"))
    assert hit >= 3
    for case, tn in [(R.GEMM_CASES[2], 0), (R.TN_CASES[1], 1)]:
        c = R.gemm_case(case[1], "exact", tn)
        f = R.gemm_tn_parts if tn else R.gemm_parts
        assert _caught(lambda: exact(f(c["a"], c["b"], case[2], shift=1), f(c["a"], c["b"], case[2]), "shift"))
    c = R.gemm_case(R.GEMM_CASES[2][1], "exact", 0)                  # last K tile dropped: invisible after no fold
    assert _caught(lambda: exact(R.gemm(c["a"][:, :256], c["b"][:256]), R.gemm(c["a"], c["b"]), "ktile"))


def test_sensitivity_slab_reduce_and_bias():
    hit = {"swap": 0, "accumulate": 0}
    for M, N in R.REDUCE_SHAPES:
        c = R.reduce_case(M, N, 3, "exact")
        for name, s_m, s_hi, s_lo, cs, size in R.reduce_perms(M, N):
            old = c["old"][:size]
            ref = R.slab_reduce(c["slab"], old, s_m, s_hi, s_lo, cs, 1, 0.5)
            if name in ("oihw", "convT", "up0"):
                hit["swap"] += _caught(lambda: exact(R.slab_reduce(c["slab"], old, s_m, s_lo, s_hi, cs, 1, 0.5,
                                                                   strict=False), ref, "s_hi / s_lo exchanged"))
            hit["accumulate"] += _caught(lambda: exact(R.slab_reduce(c["slab"], old, s_m, s_hi, s_lo, cs, 0, 0.5), ref,
                                                       "accumulate ignored"))
    assert all(hit.values()), hit
    name, shape, sp, variants = R.GEMM_CASES[0]
    c = R.gemm_case(shape, "exact", 0)
    assert (4, 0) in variants
    assert _caught(lambda: exact(R.gemm(c["a"], c["b"], c["bias"], 4, 0, wrong_bias=True),
                                 R.gemm(c["a"], c["b"], c["bias"], 4, 0), "bias[n]"))
