"""Direct tests of the LDS-halo 3x3 conv (conv3x3_halo_x3_kernel) and of the kernel-row weight gradient
(wgrad3x3_row_kernel), csrc/conv_kernels.h, in every fused form the launchers dispatch, against fp64 references on the
CPU (GPU box only).  The references, generators and predicates are tests/_conv_ref.py; tests/test_conv_refs_cpu.py holds
them to torch's fp64 autograd and asserts, for every case listed here, the conditions under which bit-equality is the
right bar.  Run this file first after touching conv_kernels.h.

The exact-data method (see _conv_ref.py).  The "exact" cases use operands that are integer multiples of 2^-3 in [-1, 1]
(weights, activations, gradients), staging coefficients that are signed powers of two or such multiples, so that every
staged operand is its own bf16 / scaled-fp16 image, every product is a multiple of one power of two and every partial
sum is an integer below 2^24 of those units: the kernel's output must equal the fp64 reference bit for bit, per
element.  No tolerance can hide a wrong halo pixel, tail column, image seam or padding value; `check` names the
offending element.  A positive shift at a padded pixel (BN-ReLU staging) and B != 0, Cc mean invstd != 0 (BN backward)
make "transform applied to the zero padding" visible.

Quantities held to a derived bound instead of bit-equality, and why:
  * the per-128-pixel column sums of squares in `stats`: the epilogue squares each stored value in fp32 (v v needs up to
    2 x the bits of v: inexact for |v| of a few hundred at a 2^-6 grid) and adds 128 of them per column: held to
    chain_bound(128, sum v^2) per 128-pixel tile.  The column sums themselves are exact on exact data.
  * "fine" cases (nterm = 1 only): BN-backward coefficients with invstd in {1/8, 1/16}, so that the kernel's bf16
    rounding of dy is not the identity; and "gauss" cases (one per entry point and arithmetic): Gaussian data.  nterm = 1:
    against the fp64 result of the operands rounded to bf16 as the kernel rounds them, per element, at
    chain_bound(K, sum|term|), K the length of the dot product (9 Cin, or the pixel count for the weight gradient), as
    test_gemm_x16 does; h3: 2e-5 max|ref| + 1e-5 (test_gpu_kernels._close).  Statistics of such cases are taken over
    the values the kernel stored, at chain_bound(128, .).
No conv output, dW, amax or max / min key of an exact case is held to anything but equality, and no dy_out of any case:
on Gaussian data too it must equal bn_bwd_elem's fp32 sequence (two fmaf, one subtraction, one product), which
_conv_ref.fma32 restates with correctly rounded fused multiply-adds.

Every output buffer is wider than its data (ld = C + 4 or C + 8, some at a nonzero channel offset) and pre-filled with
the sentinel 777 (776 as bf16); every element outside the written slice must still hold it.  Rejections are host-side
argument checks: they return hipErrorInvalidValue, launch nothing and leave the sentinel.  The one-term arithmetic has
no halo instantiation at W = 128 / 256 (halo_width_ok): the plain forward then runs the split-GEMM fallback (FWD 11-15,
18 with nterm 1, held to the same references), the BN-ReLU forward and the BN-backward dgrad reject (one rejection case
each), so the lists of (b) and (c) carry W = 128 for h3 only.

Instantiation -> cases (conv3x3_halo_x3_kernel<NT, WT, EP, ONEB, DEEP, PRE, XT>, EP = EpiStoreW<4, OT, ACC, FUSE>):
  <4, 32|64|128|256, <float>, PreNone>             FWD cases, nterm 4 (128: 11-13, 18; 256: 14, 15)
  <1, 32|64, <float>, ONEB, DEEP>                  FWD cases with Cin % 32 == 0 at W <= 64, nterm 1 (1, 5, 8, 17)
  <1, 32|64, <float>, ONEB>                        FWD cases with Cin in {16, 48} at W <= 64, nterm 1
  <.., <float, ACC>>  the load-ahead accumulate: EPI_ACCUM, W <= 64, fp32 output, no stats
                                                   FWD 3, 4, 8, 9, 17; DGRAD ACCUM cases at W <= 64 with dt 0 / 1
  generic accumulate (W = 128, or with stats, or bf16 output)
                                                   FWD 7, 12, 13, 18; DGRAD ACCUM at W = 128 (128-1-16-132) and with
                                                   bf16 out (32-1-16-132 dt 2, 64-1-48-4 dt 3)
  split-GEMM fallback (nterm 1, W >= 128)          FWD 11-15, 18, nterm 1
  several tiles per block, short last block        FWD 10
  <.., PreBnRelu, XT float|bf16>, OT float|bf16    PRE cases (dt 0-3)
  <.., PreBnBwd, XT float|bf16>, OT float|bf16     DGRAD cases (dt 0-3), with and without dy_out
  <.., <float, false, FUSE>>                       FUSED cases, kinds 1-3
wgrad3x3_row_kernel<NT, KS, PRE, PX, GT, XT>: WGRAD_CASES and SUMS_CASES; each case names its KS (last field), which
tests/test_conv_refs_cpu.py holds to the launcher's rules restated in _conv_ref.wgrad_ks; the table above WGRAD_CASES
lists which (NT, KS, dY, X) combinations are hit, and with how many splits.
"""
import numpy as np
import pytest
import torch

import _conv_ref as R
from _conv_ref import EPI_ACCUM, EPI_RELU, NT_H3, SENT, chain_bound, check, exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
INVALID = 1          # hipErrorInvalidValue
ISENT = 12345        # sentinel of int buffers


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cdm_amd
    return cdm_amd.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t, off=0):
    """device address of t (+ off elements); t stays alive until the test ends (launches are asynchronous)"""
    if t is None:
        return None
    _KEEP.append(t)
    return t.data_ptr() + off * t.element_size()


def T(a, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)
    return t.to(torch.bfloat16) if bf else t


def Hh(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().numpy().astype(np.float64)


def sent(bf):
    return float(R.bf16([SENT])[0]) if bf else SENT


def wide(a, ld, off, bf=False):
    """a [..., C] as rows of a [pixels, ld] device buffer (channel offset off), sentinel elsewhere"""
    C = a.shape[-1]
    buf = np.full((int(np.prod(a.shape[:-1])), ld), SENT)
    buf[:, off:off + C] = a.reshape(-1, C)
    return T(buf, bf)


def outbuf(rows, C, ld, off, bf=False, old=None):
    return wide(np.full((rows, C), SENT) if old is None else old.reshape(rows, C), ld, off, bf)


def take(buf, shape, off, bf=False):
    """the [.., C] slice at channel offset off of a wide buffer; everything else must still hold the sentinel"""
    a = Hh(buf)
    C = shape[-1]
    rest = np.ones(a.shape, dtype=bool)
    rest[:, off:off + C] = False
    bad = rest & (a != sent(bf))
    assert not bad.any(), f"wrote outside its slice, first at (row, column) {tuple(np.argwhere(bad)[0])}"
    return a[:, off:off + C].reshape(shape)


def untouched(buf, bf=False):
    return bool((Hh(buf) == sent(bf)).all())


def hold(got, c, mode, n, what):
    if mode == "exact":
        exact(got, c["ref"], what)
    elif mode == "h3":
        check(got, c["ref"], 2e-5 * np.abs(c["ref"]).max() + 1e-5, what)
    else:
        check(got, c["ref"], chain_bound(n, c["mag"]), what)


def mode_of(data, nterm):
    """exact data: bit-equal; "fine" BN-backward coefficients: exact under h3, bf16-rounded dy under nterm = 1"""
    if data == "exact" or (data == "fine" and nterm == NT_H3):
        return "exact", 0
    return ("h3", 0) if nterm == NT_H3 else ("chain", 1)


def check_stats(stats, stats_ld, got, Cout, mode, what):
    """stats[tile][0 | 1][stats_ld] of the stored values: sums exact on exact data (else chain_bound(128, sum|v|)), sums
    of squares chain_bound(128, sum v^2) per 128-pixel tile (the epilogue's fp32 v v is inexact); pads untouched"""
    tiles = -(-got.reshape(-1, Cout).shape[0] // 128)      # a partial last tile: the rows that exist
    a = Hh(stats).reshape(tiles, 2, stats_ld)
    assert (a[:, :, Cout:] == SENT).all(), f"{what}: stats pad written"
    s_ref, q_ref = R.tile_stats(got.reshape(-1, Cout))
    if mode == "exact":
        exact(a[:, 0, :Cout], s_ref, what + " stats sums")
    else:
        check(a[:, 0, :Cout], s_ref, chain_bound(128, R.tile_stats(np.abs(got).reshape(-1, Cout))[0]), what + " stats sums")
    check(a[:, 1, :Cout], q_ref, chain_bound(128, q_ref), what + " stats sums of squares")


def amax_of(L, buf, rows, C, ld, off):
    am = torch.zeros(1, device=DEV)
    L.cdm_amax_f32(P(buf, off), rows, C, ld, P(am), 0, _s())
    return am


def pack_weights(L, Wt, nterm, dgrad=False, dummy=False):
    """the split image of the kc = 16 packed weights of OIHW Wt: forward (K = 9 I, columns O) or, dgrad, the input
    gradient's (K = 9 O, columns I); (wx, amax_w).  dummy: zeros of the right size (rejection cases: nothing reads it)"""
    O, I = Wt.shape[:2]
    K, NN = (9 * O, I) if dgrad else (9 * I, O)
    wx = torch.zeros(((K + 15) // 16) * 3 * NN * 16, dtype=torch.bfloat16, device=DEV)
    am = torch.ones(1, device=DEV)
    if dummy:
        return wx, am
    Wd, pk = T(Wt), torch.zeros(K, NN, device=DEV)
    L.cdm_pack_conv3x3(P(Wd), P(torch.zeros(O, device=DEV)), I, O, None, None, None, None, 0.0, None if dgrad else P(pk),
                       None, P(pk) if dgrad else None, 16, _s())
    if nterm == NT_H3:
        L.cdm_amax_f32(P(pk), K, NN, NN, P(am), 0, _s())
        L.cdm_split_f16x2(P(pk), NN, K, NN, P(am), P(wx), _s())
    else:
        L.cdm_split_bf16x3(P(pk), NN, K, NN, P(wx), _s())
    return wx, am


def call(L, name, args, reject):
    """the entry point with the ordered arguments `args`; reject: through the raw symbol, must return
    hipErrorInvalidValue"""
    if reject:
        rc = L.raw(name)(*args.values())
        torch.cuda.synchronize()
        assert rc == INVALID, f"{name} returned {rc}, expected hipErrorInvalidValue"
    else:
        assert getattr(L, name)(*args.values()) == 0


def offs(N):
    """(ldx - C, x offset, ldy - C, y offset): the three-image cases address channel slices at a nonzero offset"""
    return (8, 4, 8, 4) if N == 3 else (4, 0, 4, 0)


# ----------------------------------------------------------------------------------------------------------------
# a. forward, PreNone
# ----------------------------------------------------------------------------------------------------------------
RA = EPI_RELU | EPI_ACCUM
# (W, N, Cin, Cout, flags, bias, stats + amax_y, data)
FWD_CASES = [
    (32, 1, 16, 4, 0, True, True, "exact"),              # 0  4 tiles, partial column tile
    (32, 3, 32, 36, EPI_RELU, False, False, "exact"),    # 1  12 tiles; nterm 1: DEEP
    (32, 5, 48, 132, 0, True, True, "exact"),            # 2  20 tiles, full tile + 4-column tail; 3 chunks
    (32, 3, 16, 128, EPI_ACCUM, True, False, "exact"),   # 3  ACC, full tile (the fast epilogue path)
    (32, 1, 48, 132, RA, True, False, "exact"),          # 4  ACC + relu, tail tile (bounds-checked epilogue)
    (64, 1, 32, 36, 0, False, True, "exact"),            # 5  W 64, 16 tiles; nterm 1: DEEP
    (64, 3, 16, 132, EPI_RELU, True, True, "exact"),     # 6  48 tiles, image seams inside the XCD ranges
    (64, 1, 48, 128, EPI_ACCUM, False, True, "exact"),   # 7  ACCUM with stats: the generic accumulate at W <= 64
    (64, 3, 32, 128, RA, True, False, "exact"),          # 8  ACC + relu, full tile; nterm 1: DEEP
    (64, 1, 16, 4, EPI_ACCUM, True, False, "exact"),     # 9  ACC, partial tile
    (32, 97, 16, 132, 0, True, True, "exact"),           # 10 several tiles per block, short last block (below)
    (128, 1, 16, 36, 0, True, True, "exact"),            # 11 wide rows (h3); nterm 1: the split-GEMM fallback
    (128, 3, 48, 132, EPI_ACCUM, False, False, "exact"),  # 12 generic accumulate at W = 128, 192 tiles, tail
    (128, 1, 32, 128, RA, True, True, "exact"),          # 13 generic accumulate + relu + stats, full tile
    (256, 1, 16, 36, EPI_RELU, True, False, "exact"),    # 14 W 256 (h3)
    (256, 1, 32, 132, 0, False, True, "exact"),          # 15 W 256, tail
    (32, 3, 48, 36, 0, True, True, "gauss"),             # 16 Gaussian data
    (64, 1, 32, 132, RA, True, False, "gauss"),          # 17 Gaussian data, ACC
    (128, 1, 16, 36, EPI_ACCUM, True, True, "gauss"),    # 18 Gaussian data, wide rows / fallback
]
# case 10: mtiles = 97 * 32 * 32 / 256 = 388, ntiles = ceil(132 / 128) = 2: halo_tpb = (388 * 2) / 256 = 3 (integer
# division), grid.x = ceil(388 / 3) = 130 blocks, the last one with 388 - 129 * 3 = 1 tile; 130 = 8 * 16 + 2, so XCDs 0 and
# 1 own 17 blocks and the others 16.  N H W Cin = 1.59 M elements.


def run_fwd(L, case, nterm):
    W, N, Cin, Cout, flags, bias, stats, data = case
    mode, ops = mode_of(data, nterm)
    c = R.fwd_case(W, N, Cin, Cout, flags, bias, data, ops)
    rows = N * W * W
    dx, xo, dy_, yo = offs(N)
    ldx, ldy, sld = Cin + dx, Cout + dy_, Cout + 4
    x = wide(c["x"], ldx, xo)
    wx, amw = pack_weights(L, c["Wt"], nterm)
    y = outbuf(rows, Cout, ldy, yo, old=c["old"])
    st = torch.full((rows // 128, 2, sld), SENT, device=DEV) if stats else None
    amy = torch.zeros(1, device=DEV) if stats else None
    amx = amax_of(L, x, rows, Cin, ldx, xo)
    a = dict(x=P(x, xo), N=N, H=W, W=W, Cin=Cin, ldx=ldx, wx=P(wx), amax_x=P(amx), amax_w=P(amw),
             bias=P(T(c["b"])) if bias else None, y=P(y, yo), ldy=ldy, Cout=Cout, flags=flags, stats=P(st), stats_ld=sld,
             kc=16, amax_y=P(amy), nterm=nterm, dt=0, stream=_s())
    call(L, "cdm_conv3x3_fwd_x16", a, False)
    got = take(y, (N, W, W, Cout), yo)
    hold(got, c, mode, 9 * Cin + 2, f"fwd {case} nterm {nterm}")
    if stats:
        check_stats(st, sld, got, Cout, mode, f"fwd {case} nterm {nterm}")
        assert Hh(amy)[0] == np.abs(got).max(), "amax_y"


@pytest.mark.parametrize("nterm", [4, 1])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fwd_plain(L, case, nterm):
    """cdm_conv3x3_fwd_x16 over the covering list FWD_CASES (the module docstring maps instantiations to cases): tile
    counts 4 / 12 / 20 at W = 32 (no multiple of 8 under the XCD remap), Cin 16 / 32 / 48 (DEEP on / off for nterm 1, odd
    chunk counts), Cout 4 / 36 / 128 / 132 (partial, full, full + tail), every flag combination with a dyadic old value,
    ldx > Cin, ldy > Cout.  nterm 1 at W = 128 / 256 has no halo instantiation: conv3x3_fwd_split falls through to the
    split GEMM, which must return 0 and be just as exact."""
    run_fwd(L, case, nterm)


# ----------------------------------------------------------------------------------------------------------------
# b. forward with the BN-ReLU staging, statistics and max / min keys
# ----------------------------------------------------------------------------------------------------------------
# (W, N, Cin, Cout, nterm, dt, data)
PRE_CASES = [
    (32, 1, 16, 36, 4, 0, "exact"), (32, 3, 48, 132, 4, 0, "exact"), (32, 1, 256, 36, 4, 0, "exact"),
    (64, 3, 16, 132, 4, 0, "exact"), (64, 1, 48, 36, 4, 0, "exact"), (128, 1, 16, 132, 4, 0, "exact"),
    (128, 3, 48, 36, 4, 0, "exact"),
    (32, 3, 16, 132, 1, 0, "exact"), (32, 1, 256, 36, 1, 0, "exact"), (64, 1, 48, 132, 1, 0, "exact"),
    (64, 3, 16, 36, 1, 0, "exact"),
    (32, 3, 48, 36, 1, 1, "exact"), (32, 1, 16, 132, 1, 2, "exact"), (64, 1, 48, 36, 1, 3, "exact"),
    (64, 3, 16, 132, 1, 1, "exact"), (64, 1, 16, 36, 1, 2, "exact"), (32, 3, 48, 132, 1, 3, "exact"),
    (32, 3, 48, 36, 4, 0, "gauss"), (64, 1, 48, 132, 1, 0, "gauss"),
]


def run_pre(L, case, mut=None, dummy_w=False):
    W, N, Cin, Cout, nterm, dt, data = case
    mode, ops = mode_of(data, nterm)
    c = R.pre_case(W, N, Cin, Cout, dt, data, ops)
    rows = N * W * W
    dx, xo, dy_, yo = offs(N)
    ldx, ldy, sld, mld = Cin + dx, Cout + dy_, Cout + 4, Cout + 4
    xb, yb = bool(dt & 1), bool(dt & 2)
    x = wide(c["x"], ldx, xo, xb)
    wx, amw = pack_weights(L, c["Wt"], nterm, dummy=dummy_w)
    y = outbuf(rows, Cout, ldy, yo, yb)
    st = torch.full((rows // 128, 2, sld), SENT, device=DEV)
    amy = torch.zeros(1, device=DEV)
    ymm = torch.full((2, mld), ISENT, dtype=torch.int32, device=DEV)
    L.cdm_fill_i32(P(ymm), Cout, R.INT_MIN, _s())
    L.cdm_fill_i32(P(ymm, mld), Cout, R.INT_MAX, _s())
    a = dict(x=P(x, xo), N=N, H=W, W=W, Cin=Cin, ldx=ldx, pre_s=P(T(c["s"])), pre_t=P(T(c["t"])), wx=P(wx),
             amax_x=P(T([np.abs(c["z"]).max()])), amax_w=P(amw), bias=P(T(c["b"])), y=P(y, yo), ldy=ldy, Cout=Cout,
             flags=0, stats=P(st), stats_ld=sld, kc=16, amax_y=P(amy), ymm=P(ymm), ymm_ld=mld, nterm=nterm, dt=dt,
             stream=_s())
    a.update(mut or {})
    call(L, "cdm_conv3x3_fwd_x16_ex", a, mut is not None)
    if mut is not None:
        assert untouched(y, yb) and untouched(st)
        return
    what = f"pre {case}"
    got = take(y, (N, W, W, Cout), yo, yb)
    hold(got, c, mode, 9 * Cin + 2, what)
    check_stats(st, sld, got, Cout, mode, what)
    assert Hh(amy)[0] == np.abs(got).max(), "amax_y"
    torch.cuda.synchronize()
    k = ymm.cpu().numpy()
    assert (k[:, Cout:] == ISENT).all(), "ymm pad written"
    assert np.array_equal(k[:, :Cout], R.ymm_keys(got)), "ymm keys"


@pytest.mark.parametrize("case", PRE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fwd_bn_relu_staged(L, case):
    """cdm_conv3x3_fwd_x16_ex with z = relu(x pre_s + pre_t) applied while staging, bias, stats, amax_y and the ordered
    max / min keys (taken over the stored values: bf16-rounded for dt & 2).  pre_t has both signs: a positive shift
    applied to a padded halo pixel would add relu(t) w to every border output.  dt 1 / 2 / 3: bf16 x in and / or bf16 y
    out (nterm 1)."""
    run_pre(L, case)


@pytest.mark.parametrize("case,mut", [
    ((32, 1, 272, 36, 4, 0, "exact"), {}),                       # Cin = 272 with pre_s (coefficients staged for <= 256)
    ((32, 1, 16, 36, 4, 0, "exact"), {"stats": None}),           # ymm without stats
    ((32, 1, 16, 36, 1, 0, "exact"), {"pre_t": None}),           # pre_s without pre_t
    ((32, 1, 16, 36, 4, 1, "exact"), {}),                        # dt != 0 with nterm 4
    ((32, 1, 16, 36, 4, 2, "exact"), {}),
    ((128, 1, 16, 36, 1, 0, "exact"), {}),                       # nterm 1 at W = 128: no halo instantiation
], ids=["cin272", "ymm_without_stats", "pre_s_without_pre_t", "dt1_h3", "dt2_h3", "w128_one_term"])
def test_fwd_bn_relu_staged_rejects(L, case, mut):
    run_pre(L, case, mut, dummy_w=True)


# ----------------------------------------------------------------------------------------------------------------
# c. BN-backward dgrad
# ----------------------------------------------------------------------------------------------------------------
# (W, N, C, Cout, flags, amax_out, dy_out, nterm, dt, data)
DGRAD_CASES = [
    (32, 1, 16, 4, 0, True, True, 4, 0, "exact"), (32, 3, 48, 36, EPI_ACCUM, False, False, 4, 0, "exact"),
    (32, 1, 256, 132, 0, False, True, 4, 0, "exact"), (64, 3, 16, 132, EPI_ACCUM, True, True, 4, 0, "exact"),
    (64, 1, 48, 36, 0, True, False, 4, 0, "exact"), (128, 1, 16, 132, EPI_ACCUM, True, True, 4, 0, "exact"),
    (128, 3, 48, 4, 0, False, True, 4, 0, "exact"), (32, 3, 48, 132, 0, True, True, 4, 0, "fine"),
    (32, 3, 16, 132, 0, True, True, 1, 0, "exact"), (32, 1, 48, 4, EPI_ACCUM, False, True, 1, 0, "exact"),
    (32, 1, 256, 36, EPI_ACCUM, True, False, 1, 0, "exact"), (64, 1, 48, 132, EPI_ACCUM, True, True, 1, 0, "exact"),
    (64, 3, 16, 36, 0, False, True, 1, 0, "exact"),
    (32, 3, 48, 36, 0, True, True, 1, 1, "exact"), (32, 1, 16, 132, EPI_ACCUM, True, True, 1, 2, "exact"),
    (64, 1, 48, 4, EPI_ACCUM, False, True, 1, 3, "exact"), (64, 3, 16, 132, 0, True, False, 1, 1, "exact"),
    (64, 1, 16, 36, 0, True, True, 1, 2, "exact"), (32, 3, 48, 132, 0, True, True, 1, 3, "exact"),
    (32, 3, 48, 132, 0, True, True, 1, 0, "fine"),
    (32, 3, 48, 36, EPI_ACCUM, True, True, 4, 0, "gauss"), (64, 1, 48, 132, 0, True, True, 1, 0, "gauss"),
]


def run_dgrad(L, case, mut=None, ldg_extra=0):
    W, N, C, Cout, flags, want_amax, want_dy, nterm, dt, data = case
    mode, ops = mode_of(data, nterm)
    c = R.dgrad_case(W, N, C, Cout, flags, dt, data, ops)
    rows = N * W * W
    dg, go, do, oo = offs(N)
    ldg, ldy, ldo = C + dg + ldg_extra, C + 8 + (4 if N == 3 else 0), Cout + do   # ldg != ldy, both > C
    gb, ob = bool(dt & 1), bool(dt & 2)
    g, y = wide(c["g"], ldg, go, gb), wide(c["y"], ldy, go, gb)
    co = [T(v) for v in c["co"]]
    wx, amw = pack_weights(L, c["Wt"], nterm, dgrad=True, dummy=mut is not None)
    out = outbuf(rows, Cout, ldo, oo, ob, old=c["old"])
    dyo = outbuf(rows, C, ldg, go, gb) if want_dy else None
    am = T([np.abs(c["g"]).max(), np.abs(c["y"]).max(), 0.0, 0.0])     # max|g|, max|y|, the dy bound, amax_out
    L.cdm_bn_bwd_amax_bound(C, *[P(v) for v in co[4:7]], P(co[2]), P(co[3]), P(am), P(am, 1), P(am, 2), _s())
    a = dict(g=P(g, go), ldg=ldg, y=P(y, go), ldy=ldy, s=P(co[0]), t=P(co[1]), mean=P(co[2]), invstd=P(co[3]), A=P(co[4]),
             B=P(co[5]), Cc=P(co[6]), N=N, H=W, W=W, C=C, wx=P(wx), amax_dy=P(am, 2), amax_w=P(amw), out=P(out, oo),
             ldo=ldo, Cout=Cout, flags=flags, amax_out=P(am, 3) if want_amax else None, dy_out=P(dyo, go), nterm=nterm,
             dt=dt, stream=_s())
    a.update(mut or {})
    call(L, "cdm_conv3x3_dgrad_x16_bnbwd_dy", a, mut is not None)
    if mut is not None:
        assert (c["old"] is not None or untouched(out, ob)) and (dyo is None or untouched(dyo, gb))
        return
    what = f"dgrad {case}"
    got = take(out, (N, W, W, Cout), oo, ob)
    hold(got, c, mode, 9 * C + 2, what)
    amh = Hh(am)
    assert amh[2] >= np.abs(c["dy32"]).max() > 0, "cdm_bn_bwd_amax_bound does not bound max|dy|"
    if want_amax:
        assert amh[3] == np.abs(got).max(), "amax_out"
    if want_dy:
        # every element once, in g's element type and at g's stride: the staged dy (rounded to bf16 for bf16 g: the
        # identity on exact data).  Gaussian data too: dy32 is the fp32 sequence of bn_bwd_elem with correctly rounded
        # fused multiply-adds (_conv_ref.fma32), so equality is the bar
        exact(take(dyo, (N, W, W, C), go, gb), R.bf16(c["dy32"]) if gb else c["dy32"], what + " dy_out")


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_dgrad_bn_bwd_staged(L, case):
    """cdm_conv3x3_dgrad_x16_bnbwd_dy: dy = A (y s + t > 0 ? g : 0) + B + Cc (y - mean) invstd staged (B != 0 and
    Cc mean invstd != 0 on every channel: a padded halo pixel that is not zeroed after the transform shows on every
    border output), the input gradient with flags 0 / ACCUM (ACC epilogue at W <= 64, generic at 128), amax_out, the
    stored dy_out, ldg != ldy, bf16 g / y and / or bf16 out (dt).  "fine": see the module docstring."""
    run_dgrad(L, case)


@pytest.mark.parametrize("case,extra", [
    ((256, 1, 16, 36, 0, True, True, 4, 0, "exact"), 0),      # W = 256: no BN-backward staging instantiation
    ((32, 1, 272, 36, 0, True, True, 4, 0, "exact"), 0),      # C = 272 > 256
    ((32, 1, 24, 36, 0, True, True, 4, 0, "exact"), 0),       # C = 24: not whole 16-channel chunks
    ((32, 1, 16, 36, 0, True, True, 1, 0, "exact"), 2),       # ldg % 4 != 0
    ((128, 1, 16, 36, 0, True, True, 1, 0, "exact"), 0),      # nterm 1 at W = 128: no halo instantiation
], ids=["w256", "c272", "c24", "ldg_unaligned", "w128_one_term"])
def test_dgrad_bn_bwd_staged_rejects(L, case, extra):
    run_dgrad(L, case, {}, ldg_extra=extra)


# ----------------------------------------------------------------------------------------------------------------
# d. eval epilogues
# ----------------------------------------------------------------------------------------------------------------
# (kind, W, Cin, Cout, var, nterm, data); kind 1: var = split; kind 2: var = 1 per-image FiLM rows (fan = fbn = Cout)
FUSED_CASES = [
    (1, 32, 16, 128, 0, 4, "exact"), (1, 64, 48, 256, 1, 4, "exact"), (1, 32, 48, 256, 3, 1, "exact"),
    (1, 64, 16, 128, 1, 1, "exact"),
    (2, 32, 48, 128, 0, 4, "exact"), (2, 64, 16, 256, 1, 4, "exact"), (2, 32, 16, 256, 1, 1, "exact"),
    (2, 64, 48, 128, 0, 1, "exact"),
    (3, 32, 16, 256, 0, 4, "exact"), (3, 64, 48, 128, 0, 4, "exact"), (3, 32, 48, 128, 0, 1, "exact"),
    (3, 64, 16, 256, 0, 1, "exact"),
    (1, 32, 48, 128, 1, 4, "gauss"), (2, 64, 16, 128, 1, 1, "gauss"), (3, 32, 16, 128, 0, 4, "gauss"),
    (3, 64, 48, 128, 0, 1, "gauss"),
]


def run_fused(L, case, mut=None):
    kind, W, Cin, Cout, var, nterm, data = case
    mode, ops = mode_of(data, nterm)
    c = R.fused_case(kind, W, Cin, Cout, var, data, ops)
    N = 3
    rows = N * W * W
    ldx, xo, ldy, yo = Cin + 8, 4, Cout + 8, 4
    orows = rows // 4 if kind == 3 else rows
    x = wide(c["x"], ldx, xo)
    wx, amw = pack_weights(L, c["Wt"], nterm, dummy=mut is not None)
    y = outbuf(orows, Cout, ldy, yo)
    amy = torch.zeros(1, device=DEV)
    amx = amax_of(L, x, rows, Cin, ldx, xo)
    fn = Cout if var else 0
    a = dict(x=P(x, xo), N=N, H=W, W=W, Cin=Cin, ldx=ldx, wx=P(wx), amax_x=P(amx), amax_w=P(amw), bias=P(T(c["b"])),
             y=P(y, yo), ldy=ldy, Cout=Cout, kc=16, amax_y=P(amy), kind=kind, sc_x=P(T(c["sc_x"])), sc_w=P(T(c["sc_w"])),
             sc_b=P(T(c["sc_b"])), split=var if kind == 1 else 0, fa=P(T(c["fa"])), fan=fn, fb=P(T(c["fb"])), fbn=fn,
             nterm=nterm, stream=_s())
    a.update(mut or {})
    call(L, "cdm_conv3x3_fwd_x16_fused", a, mut is not None)
    if mut is not None:
        assert untouched(y)
        return
    shape = (N, W // 2, W // 2, Cout) if kind == 3 else (N, W, W, Cout)
    got = take(y, shape, yo)
    hold(got, c, mode, 9 * Cin + 4, f"fused {case}")
    assert Hh(amy)[0] == np.abs(got).max(), "amax_y"
    if kind == 3 and mode == "exact":
        # the data does hold what the case is about: windows whose two largest values tie, and all-zero windows
        win = np.sort(c["v"].reshape(N, W // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4), axis=1)
        assert ((win[:, 3] == win[:, 2]) & (win[:, 3] > 0)).any() and (c["ref"] == 0).any() and (c["ref"] > 0).any()


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fwd_eval_fused(L, case):
    """cdm_conv3x3_fwd_x16_fused on v = relu(conv + bias), N = 3 images: kind 1 the shortcut add with split 0 / 1 / 3
    (which image takes the second coefficient set) and a per-pixel dyadic sc_x; kind 2 FiLM with shared (fan = fbn = 0)
    or per-image rows; kind 3 the 2 x 2 max into the [N][H/2][W/2] map at ldy > Cout, on data with ties inside windows
    and windows that are 0 after the relu.  amax_y = max of what was stored."""
    run_fused(L, case)


@pytest.mark.parametrize("case,mut", [
    ((1, 32, 16, 132, 0, 4, "exact"), {}),                       # Cout = 132: whole 128-column tiles only
    ((2, 128, 16, 128, 0, 4, "exact"), {}),                      # W = 128
    ((1, 32, 16, 128, 0, 4, "exact"), {"sc_w": None}),           # kind 1 without sc_w
    ((2, 32, 16, 128, 0, 1, "exact"), {"fb": None}),             # kind 2 without fb
], ids=["cout132", "w128", "resid_without_sc_w", "film_without_fb"])
def test_fwd_eval_fused_rejects(L, case, mut):
    run_fused(L, case, mut)


# ----------------------------------------------------------------------------------------------------------------
# e. kernel-row weight gradient
# ----------------------------------------------------------------------------------------------------------------
# (Cin, Cout, W, N, engine_splits, bn, px, nterm, dt, data, KS).  KS (K step = 16 KS pixels) is what the launcher's rules
# give for the case (_conv_ref.wgrad_ks; asserted on the CPU and again in run_wgrad): 4 for h3 and for bf16 operands at
# W % 64 == 0, else 2 at W % 32 == 0, else 1 - but a step size is taken only if the split count at that size equals the
# count sp at 16 pixels.  splits = 1 always does; engine.wgrad_splits aims at 768 blocks, i.e. 256 / 128 splits for
# 1 / 2 channel-tile pairs, which at these small N mostly leaves one 16-pixel step per split and so KS 1.  With N in
# {1, 3} the engine's count allows KS 2 only for (256, 128) / (128, 256) at 32-3 (sp 96) and 64-1 (sp 128), and KS 4
# never; the two N = 2 cases are added for that: 8192 pixels, sp 128 at every step size.
#   NT, KS: (dY, X) staged [sp]                  b = BN backward, r = relu(x x_s + x_t), - = plain
#   h3  1:  (-,-) [1, 256]  (b,r) [1, 64]  (b,r + sums) [192]
#   h3  2:  (b,-) [1]  (-,r) [1]  (b,r) [1, 96]
#   h3  4:  (b,r) [1, 128]  (b,r + sums) [1]
#   one-term  1:  (b,r) [48, 64, 192]  (-,r) [72, 192]  (b,-) [1]
#   one-term  2:  (b,r) [1, 128]  (-,-) [1]  (b,-) [128]  (-,r + sums) [128]
#   one-term  4 (bf16 operands only):  (b,r) [1, 128]  (-,r) [1]
WGRAD_CASES = [
    (128, 128, 16, 1, False, False, False, 4, 0, "exact", 1),   # 0
    (128, 128, 16, 3, True, True, True, 1, 0, "exact", 1),      # 1  sp 48
    (128, 128, 48, 1, False, True, True, 4, 0, "exact", 1),     # 2  48 % 32 != 0
    (256, 128, 48, 1, True, False, True, 1, 0, "exact", 1),     # 3  sp 72
    (128, 128, 32, 3, False, True, False, 4, 0, "exact", 2),    # 4
    (128, 256, 32, 1, True, True, True, 4, 0, "exact", 1),      # 5  sp 64 = the 16-pixel steps, but 32 32-pixel ones
    (256, 128, 32, 1, False, True, True, 1, 0, "exact", 2),     # 6
    (128, 128, 32, 3, True, False, True, 1, 0, "exact", 1),     # 7  sp 192, 96 32-pixel steps
    (128, 128, 64, 3, False, True, True, 4, 0, "exact", 4),     # 8  ks4h3, 12,288 pixels
    (128, 128, 64, 1, True, False, False, 4, 0, "exact", 1),    # 9  sp 256: 64-wide rows at 16-pixel steps
    (128, 128, 64, 1, False, True, True, 1, 0, "exact", 2),     # 10 fp32 one-term operands never take 64-pixel steps
    (128, 256, 64, 1, True, True, False, 1, 0, "exact", 2),     # 11 sp 128
    (128, 128, 64, 1, False, True, True, 1, 1, "exact", 4),     # 12 ks4: bf16 g / y
    (128, 128, 32, 3, True, True, True, 1, 2, "exact", 1),      # 13 bf16 x, sp 192
    (256, 128, 64, 1, False, False, True, 1, 3, "exact", 4),    # 14 ks4: both bf16; the raw-copy dY staging
    (128, 128, 16, 3, False, True, False, 1, 3, "exact", 1),    # 15 both bf16; the raw-copy X staging
    (128, 128, 32, 1, False, True, True, 1, 0, "fine", 2),      # 16 bf16 rounding of dy not the identity
    (128, 128, 32, 1, False, True, True, 4, 0, "gauss", 2),     # 17
    (128, 128, 32, 1, True, True, True, 1, 0, "gauss", 1),      # 18 sp 64
    (128, 128, 32, 1, False, False, True, 4, 0, "exact", 2),    # 19 h3, dY plain, X transformed
    (128, 128, 32, 1, False, False, False, 1, 0, "exact", 2),   # 20 one-term, both plain
    (128, 128, 32, 1, False, True, True, 4, 0, "exact", 2),     # 21 h3, both transforms, 32-pixel steps
    (256, 128, 32, 3, True, True, True, 4, 0, "exact", 2),      # 22 the same with sp 96
    (256, 128, 64, 1, True, True, True, 1, 0, "exact", 2),      # 23 one-term, both transforms, sp 128
    (128, 128, 32, 1, False, True, True, 1, 3, "exact", 2),     # 24 both bf16 at 32-pixel steps
    (256, 128, 64, 2, True, True, True, 4, 0, "exact", 4),      # 25 ks4h3 with sp 128 (N = 2, see above)
    (128, 256, 64, 2, True, True, True, 1, 3, "exact", 4),      # 26 ks4, both bf16, with sp 128
]
# with the producer's sums riding along (PreBnReluSums)
SUMS_CASES = [
    (128, 128, 32, 3, True, True, True, 4, 0, "exact", 1),      # sp 192
    (256, 128, 64, 1, True, False, True, 1, 0, "exact", 2),     # sp 128
    (128, 128, 64, 1, False, True, True, 4, 0, "exact", 4),     # ks4h3
]


def run_wgrad(L, case, sums=False):
    from cdm_amd.engine import wgrad_splits
    Cin, Cout, W, N, eng, bn, px, nterm, dt, data, ks = case
    mode, ops = mode_of(data, nterm)
    c = R.wgrad_case(Cin, Cout, W, N, bn, px, data, ops)
    rows = N * W * W
    gb, xb = bool(dt & 1), bool(dt & 2)
    ldg, ldy, ldx, off = Cout + 8, Cout + 4, Cin + 8, 4
    g, y, x = wide(c["g"], ldg, off, gb), wide(c["y"], ldy, 0, gb), wide(c["x"], ldx, off, xb)
    co = [T(v) for v in c["co"]]
    want = wgrad_splits(rows, Cout, 9 * Cin) if eng else 1
    sp = L.raw("cdm_gemm_splits")(rows, want)
    # the restated dispatch rules that name the case's KS agree with the library and the engine on the split counts
    assert want == (R.engine_wgrad_splits(rows, Cout, Cin) if eng else 1) and sp == R.effective_splits(rows, want)
    assert R.wgrad_ks(N, W, want, nterm, dt) == ks
    am = T([max(np.abs(c["dy"]).max(), 2.0 ** -10), max(np.abs(c["X"]).max(), 2.0 ** -10)])
    bnp = [P(y), ldy] + [P(v) for v in co] if bn else [None, 0] + [None] * 7
    slabs = []
    for with_sums in ([False, True] if sums else [False]):
        slab = torch.full((sp * Cout * 9 * Cin + 8,), SENT, device=DEV)
        xs = None
        if with_sums:
            rng = np.random.default_rng(7)
            xg = wide(R.d3(rng, (rows, Cin)), Cin + 4, 0, xb)
            xm, xi = T(R.d3(rng, Cin)), T(R.pick(rng, Cin, [1.0, 2.0]))
            # one partial per block: x_sums[(split * 3 + kernel row) * (Cout / 128) + co tile][5][Cin] (include/cdm_hip.h)
            xs = torch.full((sp * 3 * (Cout // 128) * 5 * Cin + 8,), SENT, device=DEV)
            sargs = [P(xg), Cin + 4, P(xm), P(xi), P(xs)]
        else:
            sargs = [None, 0, None, None, None]
        assert L.cdm_conv3x3_wgrad_x16_ex(P(g, off), ldg, *bnp, Cout, P(x, off), N, W, W, Cin, ldx,
                                          P(T(c["xs"])) if px else None, P(T(c["xt"])) if px else None, *sargs,
                                          P(am), P(am, 1), want, P(slab), nterm, dt, _s()) == 0
        s = Hh(slab)
        assert (s[-8:] == SENT).all(), "wrote past the end of the slab"
        slabs.append(s[:-8])
        if xs is not None:
            assert (Hh(xs)[-8:] == SENT).all(), "wrote past the end of x_sums"
    if sums:
        assert np.array_equal(slabs[0], slabs[1]), "the producer sums changed the slab"
    dW = torch.full((Cout * Cin * 9 + 8,), SENT, device=DEV)
    L.cdm_slab_reduce(P(T(slabs[0])), sp, Cout, 9 * Cin, P(dW), 9 * Cin, 1, 9, Cin, 0, 1.0, _s())
    d = Hh(dW)
    assert (d[-8:] == SENT).all()
    if mode == "exact":
        # the slab itself: its split partials are exact, so their fp64 sum is the reference, [co][tap][ci]
        tot = slabs[0].reshape(sp, Cout, 9, Cin).sum(0).transpose(0, 2, 1).reshape(Cout, Cin, 3, 3)
        exact(tot, c["ref"], f"wgrad {case} slab")
    hold(d[:-8].reshape(Cout, Cin, 3, 3), c, mode, rows + sp + 2, f"wgrad {case}")


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_wgrad_row(L, case):
    """cdm_conv3x3_wgrad_x16_ex reduced with cdm_slab_reduce: the four staging combinations {dY plain | BN backward} x
    {X plain | relu(x x_s + x_t)} in both arithmetics, bf16 operands (dt), the 16- / 32- / 64-pixel K steps (the table
    above WGRAD_CASES: which combination runs at which step, with how many splits), splits = 1 and
    engine.wgrad_splits, ldg, ldy, ldx > C.  Each dW element against the fp64 weight gradient of the staged operands;
    exact data sums up to 12,288 pixels of products within the budget tests/test_conv_refs_cpu.py asserts.  x_t has
    both signs and differs per channel: a coefficient of the wrong channel changes z."""
    run_wgrad(L, case)


@pytest.mark.parametrize("case", SUMS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_wgrad_row_with_producer_sums(L, case):
    """with x_sums the slab is bit-identical to the one without (the existing assertion of
    test_producer_bn_sums_in_wgrad), and equals the reference"""
    run_wgrad(L, case, sums=True)
