"""Direct tests of the contraction code outside the LDS-halo / kernel-row kernels: all of csrc/gemm_f32.hip and the kernels
its launchers pick from csrc/conv_kernels.h, against fp64 references on the CPU (GPU box only).  The references, the
generators, the case lists and the restated dispatch predicates are tests/_gemm_ref.py; tests/test_gemm_refs_cpu.py holds
them to torch's fp64 operators and asserts, for every exact case listed there, the conditions under which bit-equality
is the right bar, the path each case takes, and that the data sees the error classes the cases are about.  Run this
file after touching gemm_f32.hip or the GEMM part of conv_kernels.h.

The exact-data method is the halo file's (tests/test_gpu_halo_ops.py, tests/_conv_ref.py): operands are integer
multiples of 2^-3 in [-1, 1] with max|.| = 1 (so cdm_amax_f32 gives 1 and the h3 scale is 2^13), every product a
multiple of 2^-6, every partial sum an integer below 2^24 units: the output, every split's slab and every amax must
equal the fp64 reference bit for bit, per element (`exact` names the offending element).  Held to a derived bound
instead: the per-128-pixel column sums of squares of `stats` (chain_bound(128, sum v^2): the epilogue's fp32 v v is
inexact), and the Gaussian cases (one per entry point and arithmetic): fp32 kernels and nterm = 1 (against the fp64
result of the bf16-rounded operands) per element within chain_bound(K, sum|term|); h3 2e-5 max|ref| + 1e-5; the
split-bf16 forms nterm 6 / 3 chain_bound(6 K | 3 K, .) plus the dropped cross terms (5 x 2^-24 | 4 x 2^-16 of
sum|term|: x = hi + mid + lo with |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|); cdm_slab_reduce chain_bound(splits, sum|slab|).

Every output is a wide buffer (ld = C + 4, or C + 8 at channel offset 4) pre-filled with the sentinel, every input has
ld > C; `take` asserts that nothing outside the slice was written.  Slabs have room for one split more than is used,
sentinel-filled.  Rejections go through the raw symbol: hipErrorInvalidValue, nothing launched, the sentinel intact.

Kernel / instantiation -> cases (names as in _gemm_ref.py; G = the Gaussian case of the list):
  gemm_f32_kernel<LdDenseA, LdDenseB, EpiConvT2x2>            cdm_convT2x2_fwd: F0-F5, FG
  gemm_f32_kernel<LdConvT2x2GatherA, LdDenseB, EpiStore>      cdm_convT2x2_dgrad: D0-D4 x flags 0 / ACCUM / RELU|ACCUM, DG
  gemm_f32_kernel<LdDenseAT, LdConvT2x2GatherB, EpiStore>     cdm_convT2x2_wgrad: W0-W4, WG (split-K slabs)
  gemm_f32_kernel<LdIm2colA<0, KC>, LdDenseB, EpiStore, remap>        cdm_conv3x3_fwd: C0 (kc 0), C1, C4 (5 tiles), CG
  gemm_f32_kernel<LdIm2colA<128, KC>, ..>                     C2 (ACCUM), C5 (11 tiles); kc 0 and 16, forward and dgrad
  gemm_f32_kernel<LdIm2colA<128, KC, 64>, ..>                 C3 (64 tiles, image seam, stats)
  gemm_f32_kernel<LdDenseAT, LdIm2colB, EpiStore>             cdm_conv3x3_wgrad: C0-C5 x splits 1 / 7
  gemm_f32_kernel<LdDenseA, LdDenseB, EpiStore>               cdm_gemm_f32: G0 (bias_mod, flags), G1, G2 (9 splits), GG
  gemm_f32_kernel<LdDenseAT, LdDenseB, EpiStore>              cdm_gemm_tn_f32: TN0, TN1, TNG
  gemm_x3_kernel<StageRowK<LdDenseA>, StagePre, EpiConvT2x2>  cdm_convT2x2_fwd_x16: F0, F1 (never deep), F2-F5 with
                                                              CDM_CONVT_DEEP=0; nterm 4 and 1
  gemm_x3_kernel<StageRowK<LdConvT2x2GatherA>, StagePre, EpiStore>    cdm_convT2x2_dgrad_x16: D0, D3, D1 / D2 / D4 with
                                                              CDM_CONVT_DEEP=0; nterm 4 and 1
  gemm_x3_kernel<StageColK<LdDenseAT>, StageColK<LdConvT2x2GatherB>>  cdm_convT2x2_wgrad_x16: W0, W4; nterm 4 and 1
  gemm_x3_kernel<StageRowK<LdIm2colA<..>>, StagePre, EpiStore> (nterm 6, 3, 1)   cdm_conv3x3_fwd_x3: C0-C2, C4, C5, CG
                                                              (C3 at kc 16 runs the LDS-halo kernel in these arithmetics)
  gemm_x3_kernel<StageColK<LdDenseAT>, StageColK<LdIm2colB>>  cdm_conv3x3_wgrad_x3: C0, C1, C4 (C2, C3, C5: the
                                                              kernel-row kernel in nterm 6 / 3 / 1)
  gemm_deep_kernel<h3 | bf16, DeepDenseA, EpiConvT2x2>        F2 (nwg 3), F3 (2 x 3), F4 (nwg 11), F5 (ldx = Cin + 8)
  gemm_deep_kernel<h3 | bf16, DeepConvT2x2GatherA, EpiStore>  D1 (nwg 3), D2 (1 x 2, sub-pixel boundaries), D4 (nwg 11),
                                                              DG; each with the three flag sets
  convT2x2_wgrad_tr_kernel<h3 | bf16>                         W1 (grid 4 / 8), W2 (grid 12 / 20, image seams), W3 (gx 2), WG
  slab_reduce_kernel                                          every (M, N) at splits < 8, N = 6 at every split count
  slab_reduce4_kernel                                         N % 4 == 0 at splits 8, 9, 16, 17, 24; partly empty last
                                                              block at (5, 36) and (3, 8)
"""
import os

import numpy as np
import pytest
import torch

import _gemm_ref as R
from _gemm_ref import EPI_ACCUM, EPI_RELU, NT_H3, SENT, chain_bound, check, exact
from test_gpu_halo_ops import (DEV, INVALID, Hh, L, P, T, _release, _s, amax_of, call, check_stats,  # noqa: F401
                               outbuf, take, untouched, wide)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
X16 = (NT_H3, 1)
DEEP_ENV = "CDM_CONVT_DEEP"


def hold(got, ref, mag, data, arith, n, what):
    """exact data: equality; Gaussian data: the bound of the arithmetic (module docstring); n = the dot product's
    length, mag = sum|term|"""
    if data == "exact":
        exact(got, ref, what)
    elif arith == NT_H3:
        check(got, ref, 2e-5 * np.abs(ref).max() + 1e-5, what)
    elif arith == 6:
        check(got, ref, chain_bound(6 * n, mag) + 5 * U * mag, what)
    elif arith == 3:
        check(got, ref, chain_bound(3 * n, mag) + 4 * 2.0 ** -16 * mag, what)
    else:
        check(got, ref, chain_bound(n, mag), what)


def ops_of(data, arith):
    """1: the reference takes the operands rounded to bf16 (Gaussian data in the one-term arithmetic)"""
    return 1 if (data != "exact" and arith == 1) else 0


def out_ld(name):
    """(ld - C, channel offset) of a case's outputs: odd-numbered cases write a slice at offset 4 of a C + 8 buffer"""
    return (8, 4) if name[-1] in "13579" else (4, 0)


def split16(L, w, K, NN, nterm):
    """the split image of the contiguous device matrix w [K][NN] for the arithmetic nterm, and max|w| (h3)"""
    wx = torch.zeros(((K + 15) // 16) * 3 * NN * 16, dtype=torch.bfloat16, device=DEV)
    am = torch.ones(1, device=DEV)
    if nterm == NT_H3:
        L.cdm_amax_f32(P(w), K, NN, NN, P(am), 0, _s())
        L.cdm_split_f16x2(P(w), NN, K, NN, P(am), P(wx), _s())
    else:
        L.cdm_split_bf16x3(P(w), NN, K, NN, P(wx), _s())
    return wx, am


def pack_convT(L, Wt):
    """(wt [Cin][4 Cout], wtT [4 Cout][Cin]) from cdm_pack_convT, held to the layout the references assume"""
    Ci, Co = Wt.shape[:2]
    wt, wtT = torch.zeros(Ci, 4 * Co, device=DEV), torch.zeros(4 * Co, Ci, device=DEV)
    L.cdm_pack_convT(P(T(Wt)), Ci, Co, 4, P(wt), P(wtT), _s())
    exact(Hh(wt), R.convT_pack(Wt), "cdm_pack_convT wt")
    exact(Hh(wtT), R.convT_pack(Wt).T, "cdm_pack_convT wtT")
    return wt, wtT


def deep_modes(eligible):
    """the environment settings a deep-eligible x16 case runs under: unset (the two-deep prefetch kernel) and
    CDM_CONVT_DEEP=0 (gemm_x3); other cases run once"""
    return (None, "0") if eligible else (None,)


class deep_env:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        os.environ.pop(DEEP_ENV, None)
        if self.v is not None:
            os.environ[DEEP_ENV] = self.v

    def __exit__(self, *a):
        os.environ.pop(DEEP_ENV, None)


def sentinel_slab(n, sp):
    """room for one split more than is used"""
    return torch.full(((sp + 1) * n,), SENT, device=DEV)


def slab_parts(slab, sp, M, N, what):
    s = Hh(slab).reshape(sp + 1, M, N)
    assert (s[sp] == SENT).all(), f"{what}: wrote past the last split's slab"
    return s[:sp]


# ----------------------------------------------------------------------------------------------------------------
# ConvT 2x2 forward
# ----------------------------------------------------------------------------------------------------------------
def run_convT_fwd(L, case, data, mut=None):
    name, shape, dld, xo = case
    N, H, W, Ci, Co = shape
    rows, orows = N * H * W, 4 * N * H * W
    ldx = Ci + dld
    dly, yo = out_ld(name)
    ldy = Co + dly
    c0 = R.convT_case(shape, data, 0)
    x = wide(c0["x"], ldx, xo)
    wt, _ = pack_convT(L, c0["Wt"])
    bias = T(c0["b"])
    amx = amax_of(L, x, rows, Ci, ldx, xo)
    if data == "exact":
        assert Hh(amx)[0] == 1.0
    if mut is not None:                                       # a rejection: nothing may be written
        y, am = outbuf(orows, Co, ldy, yo), torch.full((1,), SENT, device=DEV)
        wx, amw = split16(L, wt, Ci, 4 * Co, NT_H3)
        if mut.get("f32"):
            a = dict(x=P(x, xo), N=N, H=H, W=W, Cin=Ci, ldx=ldx, wpk=P(wt), bias=P(bias), y=P(y, yo), ldy=ldy, Cout=Co,
                     amax=P(am), stream=_s())
            ent = "cdm_convT2x2_fwd"
        else:
            a = dict(x=P(x, xo), N=N, H=H, W=W, Cin=Ci, ldx=ldx, wx=P(wx), amax_x=P(amx), amax_w=P(amw), bias=P(bias),
                     y=P(y, yo), ldy=ldy, Cout=Co, amax_y=P(am), nterm=NT_H3, stream=_s())
            ent = "cdm_convT2x2_fwd_x16"
        a.update({k: v for k, v in mut.items() if k != "f32"})
        call(L, ent, a, True)
        assert untouched(y) and Hh(am)[0] == SENT
        return
    eligible = R.deep_fwd(shape, ldx)
    for arith in ("f32",) + X16:
        c = R.convT_case(shape, data, ops_of(data, arith))
        if arith != "f32":
            wx, amw = split16(L, wt, Ci, 4 * Co, arith)
        for deep in deep_modes(eligible and arith != "f32"):
            # with bias from a clear maximum, without bias from a seed below the result's, with bias from one above
            for use_bias, seed in ((True, 0.0), (False, 0.375), (True, 4096.0)):
                what = f"convT fwd {name} {arith} deep {deep} bias {use_bias}"
                y, am = outbuf(orows, Co, ldy, yo), T([seed])
                bp = P(bias) if use_bias else None
                with deep_env(deep):
                    if arith == "f32":
                        L.cdm_convT2x2_fwd(P(x, xo), N, H, W, Ci, ldx, P(wt), bp, P(y, yo), ldy, Co, P(am), _s())
                    else:
                        h3 = arith == NT_H3
                        L.cdm_convT2x2_fwd_x16(P(x, xo), N, H, W, Ci, ldx, P(wx), P(amx) if h3 else None,
                                               P(amw) if h3 else None, bp, P(y, yo), ldy, Co, P(am), arith, _s())
                got = take(y, (N, 2 * H, 2 * W, Co), yo)
                ref = c["y"] + c["b"] if use_bias else c["y"]
                hold(got, ref, c["y_mag"] + (np.abs(c["b"]) if use_bias else 0.0), data, arith, Ci + 2, what)
                assert Hh(am)[0] == max(seed, np.abs(got).max()), what + ": amax"


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c[0])
def test_convT2x2_fwd(L, case):
    """cdm_convT2x2_fwd and cdm_convT2x2_fwd_x16 (nterm 4 and 1; deep-eligible cases with CDM_CONVT_DEEP unset and 0),
    each form against the fp64 reference on its own, with and without bias, the running maximum from a clear and from
    a nonzero seed: max(seed, max|stored|)"""
    run_convT_fwd(L, case, "exact")


def test_convT2x2_fwd_gauss(L):
    run_convT_fwd(L, R.FWD_GAUSS, "gauss")


@pytest.mark.parametrize("shape,mut", [
    ((1, 4, 8, 18, 8), {}), ((1, 4, 8, 16, 6), {}), ((1, 4, 8, 16, 8), {"nterm": 2}), ((1, 4, 8, 16, 8), {"amax_x": None}),
    ((1, 4, 8, 16, 8), {"amax_w": None}), ((1, 4, 8, 18, 8), {"f32": True}), ((1, 4, 8, 16, 6), {"f32": True}),
], ids=["cin18", "cout6", "nterm2", "h3_no_amax_x", "h3_no_amax_w", "f32_cin18", "f32_cout6"])
def test_convT2x2_fwd_rejects(L, shape, mut):
    run_convT_fwd(L, ("R0", shape, 2 if shape[3] % 4 else 4, 0), "exact", mut)


# ----------------------------------------------------------------------------------------------------------------
# ConvT 2x2 input gradient
# ----------------------------------------------------------------------------------------------------------------
def run_convT_dgrad(L, case, data):
    name, shape, dld, yo = case
    N, H, W, Ci, Co = shape
    rows, orows = N * H * W, 4 * N * H * W
    lddy = Co + dld
    dlx, xo = out_ld(name)
    lddx = Ci + dlx
    c0 = R.convT_case(shape, data, 0)
    dy = wide(c0["dy"], lddy, yo)
    _, wtT = pack_convT(L, c0["Wt"])
    amg = amax_of(L, dy, orows, Co, lddy, yo)
    eligible = R.deep_dgrad(shape, lddy)
    for arith in ("f32",) + X16:
        c = R.convT_case(shape, data, ops_of(data, arith))
        if arith != "f32":
            wx, amw = split16(L, wtT, 4 * Co, Ci, arith)
        for deep in deep_modes(eligible and arith != "f32"):
            for flags in R.DGRAD_FLAGS:
                what = f"convT dgrad {name} {arith} deep {deep} flags {flags}"
                old = c["old"] if flags & EPI_ACCUM else None
                dx = outbuf(rows, Ci, lddx, xo, old=old)
                with deep_env(deep):
                    if arith == "f32":
                        L.cdm_convT2x2_dgrad(P(dy, yo), N, H, W, Co, lddy, P(wtT), P(dx, xo), lddx, Ci, flags, _s())
                    else:
                        h3 = arith == NT_H3
                        L.cdm_convT2x2_dgrad_x16(P(dy, yo), N, H, W, Co, lddy, P(wx), P(amg) if h3 else None,
                                                 P(amw) if h3 else None, P(dx, xo), lddx, Ci, flags, arith, _s())
                got = take(dx, (N, H, W, Ci), xo)
                mag = c["dx_mag"] + (np.abs(old) if old is not None else 0.0)
                hold(got, R.epilogue(c["dx"], flags, old), mag, data, arith, 4 * Co + 2, what)


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=lambda c: c[0])
def test_convT2x2_dgrad(L, case):
    """cdm_convT2x2_dgrad and cdm_convT2x2_dgrad_x16 (nterm 4 and 1, deep on / off) with flags 0, ACCUM and
    RELU | ACCUM on a dyadic old value: every form against the fp64 reference, not against another form"""
    run_convT_dgrad(L, case, "exact")


def test_convT2x2_dgrad_gauss(L):
    run_convT_dgrad(L, R.DGRAD_GAUSS, "gauss")


# ----------------------------------------------------------------------------------------------------------------
# ConvT 2x2 weight gradient
# ----------------------------------------------------------------------------------------------------------------
def run_convT_wgrad(L, case, data, reject=False):
    name, shape, splits_list = case
    N, H, W, Ci, Co = shape
    K, NN = N * H * W, 4 * Co
    ldx, lddy, xo = Ci + 8, Co + 4, 4
    c0 = R.convT_case(shape, data, 0)
    x, dy = wide(c0["x"], ldx, xo), wide(c0["dy"], lddy, 0)
    amx, amg = amax_of(L, x, K, Ci, ldx, xo), amax_of(L, dy, 4 * K, Co, lddy, 0)
    if reject:
        slab = sentinel_slab(Ci * NN, 1)
        a = dict(x=P(x, xo), N=N, H=H, W=W, Cin=Ci, ldx=ldx, dy=P(dy), Cout=Co, lddy=lddy, amax_x=P(amx), amax_dy=P(amg),
                 splits=1, slab=P(slab), nterm=NT_H3, stream=_s())
        call(L, "cdm_convT2x2_wgrad_x16", a, True)
        assert untouched(slab)
        return
    for splits in splits_list:
        sp = L.raw("cdm_gemm_splits")(K, splits)
        ranges = R.split_ranges(K, splits)
        assert sp == len(ranges)
        for arith in ("f32",) + X16:
            what = f"convT wgrad {name} {arith} splits {splits}"
            c = R.convT_case(shape, data, ops_of(data, arith))
            parts = R.convT_wgrad_parts(c["xq"], c["dyq"], splits)
            mags = R.convT_wgrad_parts(np.abs(c["xq"]), np.abs(c["dyq"]), splits)
            slab = sentinel_slab(Ci * NN, sp)
            if arith == "f32":
                L.cdm_convT2x2_wgrad(P(x, xo), N, H, W, Ci, ldx, P(dy), Co, lddy, splits, P(slab), _s())
            else:
                h3 = arith == NT_H3
                L.cdm_convT2x2_wgrad_x16(P(x, xo), N, H, W, Ci, ldx, P(dy), Co, lddy, P(amx) if h3 else None,
                                         P(amg) if h3 else None, splits, P(slab), arith, _s())
            got = slab_parts(slab, sp, Ci, NN, what)
            for z, (k0, k1) in enumerate(ranges):
                hold(got[z], parts[z], mags[z], data, arith, k1 - k0 + 2, f"{what} split {z}")
            dW = torch.full((Ci * NN + 8,), SENT, device=DEV)
            L.cdm_slab_reduce(P(slab), sp, Ci, NN, P(dW), NN, 1, 4, Co, 0, 1.0, _s())
            d = Hh(dW)
            assert (d[-8:] == SENT).all()
            ref = parts.sum(0).reshape(Ci, 2, 2, Co).transpose(0, 3, 1, 2)          # [Cin][Cout][2][2]
            hold(d[:-8].reshape(Ci, Co, 2, 2), ref, mags.sum(0).reshape(Ci, 2, 2, Co).transpose(0, 3, 1, 2), data, arith,
                 K + sp + 2, what + " folded")


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: c[0])
def test_convT2x2_wgrad(L, case):
    """cdm_convT2x2_wgrad and cdm_convT2x2_wgrad_x16 (nterm 4 and 1): every split's slab against the partial over its
    own input-pixel range (a wrong range that still covers K once fails), the slab after the last split untouched,
    then the cdm_slab_reduce fold in [Cin][Cout][2][2] order against dW"""
    run_convT_wgrad(L, case, "exact")


def test_convT2x2_wgrad_gauss(L):
    run_convT_wgrad(L, R.WGRAD_GAUSS, "gauss")


def test_convT2x2_wgrad_x16_rejects_w4(L):
    run_convT_wgrad(L, ("R0", (1, 4, 4, 16, 8), (1,)), "exact", reject=True)


# ----------------------------------------------------------------------------------------------------------------
# fp32 3x3 conv and its split-bf16 siblings
# ----------------------------------------------------------------------------------------------------------------
def pack3x3(L, Wt, kc, dgrad):
    """the kc-ordered packed weights of OIHW Wt: forward [9 I][O] or, dgrad, the input gradient's [9 O][I]"""
    O, I = Wt.shape[:2]
    K, NN = (9 * O, I) if dgrad else (9 * I, O)
    pk = torch.zeros(K, NN, device=DEV)
    L.cdm_pack_conv3x3(P(T(Wt)), P(torch.zeros(O, device=DEV)), I, O, None, None, None, None, 0.0,
                       None if dgrad else P(pk), None, P(pk) if dgrad else None, kc, _s())
    return pk


def run_conv_fwd(L, case, data):
    name, shape, kcs, flags, use_bias, stats = case
    N, H, W, Ci, Co = shape
    rows = N * H * W
    tiles = -(-rows // 128)
    ldx, xo = Ci + 4, 0
    dly, yo = out_ld(name)
    c0 = R.conv_case(shape, data, 0)
    x, gy = wide(c0["x"], ldx, xo), wide(c0["gy"], Co + 8, 4)
    bias = T(c0["b"])
    forms = [("f32", kc) for kc in kcs] + [(nt, kcs[-1]) for nt in (6, 3, 1)]
    for arith, kc in forms:
        c = R.conv_case(shape, data, ops_of(data, arith))
        what = f"conv3x3 fwd {name} {arith} kc {kc}"
        b = c["b"] if use_bias else None
        old = c["old"] if flags & EPI_ACCUM else None
        ldy, sld = Co + dly, Co + 4
        y = outbuf(rows, Co, ldy, yo, old=old)
        st = torch.full((tiles, 2, sld), SENT, device=DEV) if stats else None
        wpk = pack3x3(L, c0["Wt"], kc, False)
        if arith == "f32":
            L.cdm_conv3x3_fwd(P(x, xo), N, H, W, Ci, ldx, P(wpk), P(bias) if use_bias else None, P(y, yo), ldy, Co, flags,
                              P(st), sld, kc, _s())
        else:
            wx, _ = split16(L, wpk, 9 * Ci, Co, arith)
            L.cdm_conv3x3_fwd_x3(P(x, xo), N, H, W, Ci, ldx, P(wx), P(bias) if use_bias else None, P(y, yo), ldy, Co,
                                 flags, P(st), sld, kc, arith, _s())
        got = take(y, (N, H, W, Co), yo)
        mag = c["y_mag"] + (np.abs(b) if use_bias else 0.0) + (np.abs(old) if old is not None else 0.0)
        hold(got, R.epilogue(c["y"], flags, old, b), mag, data, arith, 9 * Ci + 3, what)
        if stats:
            check_stats(st, sld, got, Co, "exact" if data == "exact" else "chain", what)
        # the input gradient: the same kernel on gy with the flipped weights wdg (chunked over Cout when kc = 16)
        kcd = kc if (kc == 0 or Co % 16 == 0) else 0
        wdg = pack3x3(L, c0["Wt"], kcd, True)
        dx = outbuf(rows, Ci, Ci + dly, yo)
        if arith == "f32":
            L.cdm_conv3x3_fwd(P(gy, 4), N, H, W, Co, Co + 8, P(wdg), None, P(dx, yo), Ci + dly, Ci, 0, None, 0, kcd, _s())
        else:
            wdx, _ = split16(L, wdg, 9 * Co, Ci, arith)
            L.cdm_conv3x3_fwd_x3(P(gy, 4), N, H, W, Co, Co + 8, P(wdx), None, P(dx, yo), Ci + dly, Ci, 0, None, 0, kcd,
                                 arith, _s())
        hold(take(dx, (N, H, W, Ci), yo), c["dx"], c["dx_mag"], data, arith, 9 * Co + 2, what + " as dgrad")


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c[0])
def test_conv3x3_fwd(L, case):
    """cdm_conv3x3_fwd (kc 0 and 16) and cdm_conv3x3_fwd_x3 (nterm 6, 3, 1: on exact data the mid and lo terms are
    zero, so all must equal the reference), as the forward with the case's flags / bias / stats and, with wdg, as the
    input gradient.  stats: per-tile sums exact, sums of squares chain_bound(128, .), stats_ld = Cout + 4 with the pad
    untouched, a partial last tile summing the rows that exist."""
    run_conv_fwd(L, case, "exact")


def test_conv3x3_fwd_gauss(L):
    run_conv_fwd(L, R.CONV_GAUSS, "gauss")


def run_conv_wgrad(L, case, data):
    name, shape = case[0], case[1]
    N, H, W, Ci, Co = shape
    K, NN = N * H * W, 9 * Ci
    ldx, lddy = Ci + 8, Co + 4
    c0 = R.conv_case(shape, data, 0)
    x, gy = wide(c0["x"], ldx, 4), wide(c0["gy"], lddy, 0)
    for splits in R.CONV_WGRAD_SPLITS:
        sp = L.raw("cdm_gemm_splits")(K, splits)
        ranges = R.split_ranges(K, splits)
        assert sp == len(ranges)
        refs = {}
        for arith in ("f32", 6, 3, 1):
            what = f"conv3x3 wgrad {name} {arith} splits {splits}"
            ops = ops_of(data, arith)
            if ops not in refs:
                c = R.conv_case(shape, data, ops)
                refs[ops] = (R.conv3x3_wgrad_parts(c["gq"], c["xq"], splits),
                             R.conv3x3_wgrad_parts(np.abs(c["gq"]), np.abs(c["xq"]), splits) if data != "exact" else None)
            parts, mags = refs[ops]
            slab = sentinel_slab(Co * NN, sp)
            if arith == "f32":
                L.cdm_conv3x3_wgrad(P(gy), lddy, Co, P(x, 4), N, H, W, Ci, ldx, splits, P(slab), _s())
            else:
                L.cdm_conv3x3_wgrad_x3(P(gy), lddy, Co, P(x, 4), N, H, W, Ci, ldx, splits, P(slab), arith, _s())
            got = slab_parts(slab, sp, Co, NN, what)
            for z, (k0, k1) in enumerate(ranges):
                hold(got[z], parts[z], None if mags is None else mags[z], data, arith, k1 - k0 + 2, f"{what} split {z}")
            dW = torch.full((Co * NN + 8,), SENT, device=DEV)
            L.cdm_slab_reduce(P(slab), sp, Co, NN, P(dW), NN, 1, 9, Ci, 0, 1.0, _s())
            d = Hh(dW)
            assert (d[-8:] == SENT).all()
            hold(d[:-8].reshape(Co, Ci, 3, 3), R.slab_to_oihw(parts.sum(0), Ci),
                 None if mags is None else R.slab_to_oihw(mags.sum(0), Ci), data, arith, K + sp + 2, what + " folded")


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c[0])
def test_conv3x3_wgrad(L, case):
    """cdm_conv3x3_wgrad and cdm_conv3x3_wgrad_x3 (nterm 6, 3, 1) at splits 1 and 7: each split's slab against the
    partial over its pixel range, then the OIHW fold"""
    run_conv_wgrad(L, case, "exact")


def test_conv3x3_wgrad_gauss(L):
    run_conv_wgrad(L, R.CONV_GAUSS, "gauss")


# ----------------------------------------------------------------------------------------------------------------
# dense GEMMs
# ----------------------------------------------------------------------------------------------------------------
def run_gemm(L, case, data, mut=None):
    name, (M, K, N), splits, variants = case
    lda, ldb, ldc = K + 4, N + 4, N + 4
    c = R.gemm_case((M, K, N), data, 0)
    a, b, bias = wide(c["a"], lda, 0), wide(c["b"], ldb, 0), T(c["bias"])
    mag0 = np.abs(c["a"]) @ np.abs(c["b"])
    if mut is not None:
        out, slab = outbuf(M, N, ldc, 0), sentinel_slab(M * N, 1)
        args = dict(a=P(a), lda=lda, M=M, K=K, b=P(b), ldb=ldb, N=N, c=P(out), ldc=ldc, bias=P(bias), bias_mod=N, flags=0,
                    splits=1, slab=P(slab), stream=_s())
        args.update(mut)
        call(L, "cdm_gemm_f32", args, True)
        assert untouched(out) and untouched(slab)
        return
    sp = L.raw("cdm_gemm_splits")(K, splits)
    ranges = R.split_ranges(K, splits)
    assert sp == len(ranges)
    if sp > 1:                                                # raw partials into the slab, c unwritten, then the fold
        out, slab = outbuf(M, N, ldc, 0), sentinel_slab(M * N, sp)
        L.cdm_gemm_f32(P(a), lda, M, K, P(b), ldb, N, P(out), ldc, P(bias), N, 0, splits, P(slab), _s())
        assert untouched(out), f"gemm {name}: c written by a split-K launch"
        got = slab_parts(slab, sp, M, N, f"gemm {name}")
        parts = R.gemm_parts(c["a"], c["b"], splits)
        mags = R.gemm_parts(np.abs(c["a"]), np.abs(c["b"]), splits)
        for z, (k0, k1) in enumerate(ranges):
            hold(got[z], parts[z], mags[z], data, "f32", k1 - k0 + 2, f"gemm {name} split {z}")
        L.cdm_slab_reduce(P(slab), sp, M, N, P(out), ldc, 0, 1, N, 0, 1.0, _s())
        hold(take(out, (M, N), 0), R.gemm(c["a"], c["b"]), mag0, data, "f32", K + sp + 2, f"gemm {name} folded")
    for bias_mod, flags in variants:
        what = f"gemm {name} bias_mod {bias_mod} flags {flags}"
        old = c["old"] if flags & EPI_ACCUM else None
        out, slab = outbuf(M, N, ldc, 0, old=old), sentinel_slab(M * N, 1)
        L.cdm_gemm_f32(P(a), lda, M, K, P(b), ldb, N, P(out), ldc, P(bias) if bias_mod else None, bias_mod, flags, 1,
                       P(slab), _s())
        bz = c["bias"] if bias_mod else None
        ref = R.gemm(c["a"], c["b"], bz, max(bias_mod, 1), flags, old)
        mag = mag0 + (np.abs(bz[np.arange(N) % bias_mod]) if bias_mod else 0.0) + (np.abs(old) if old is not None else 0.0)
        hold(take(out, (M, N), 0), ref, mag, data, "f32", K + 3, what)
        assert untouched(slab), what + ": slab written by a one-split launch"


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=lambda c: c[0])
def test_gemm_f32(L, case):
    """cdm_gemm_f32 at lda = K + 4, ldb = N + 4, ldc = N + 4: bias_mod N and 4 (and no bias), flags 0 / RELU / ACCUM, M
    and N tails, K tails; split K: every slab against the partial of its own K range, c untouched, then the fold"""
    run_gemm(L, case, "exact")


def test_gemm_f32_gauss(L):
    run_gemm(L, R.GEMM_GAUSS, "gauss")


@pytest.mark.parametrize("shape", [(5, 38, 132), (5, 36, 130)], ids=["k38", "n130"])
def test_gemm_f32_rejects(L, shape):
    run_gemm(L, ("R0", shape, 1, []), "exact", {})


def run_gemm_tn(L, case, data, reject=False):
    name, (M, K, N), splits = case
    lda, ldb = M + 4, N + 4
    c = R.gemm_case((M, K, N), data, 1)
    a, b = wide(c["a"], lda, 0), wide(c["b"], ldb, 0)
    if reject:
        slab = sentinel_slab(M * N, 1)
        args = dict(a=P(a), lda=lda, M=M, K=K, b=P(b), ldb=ldb, N=N, splits=1, slab=P(slab), stream=_s())
        call(L, "cdm_gemm_tn_f32", args, True)
        assert untouched(slab)
        return
    sp = L.raw("cdm_gemm_splits")(K, splits)
    ranges = R.split_ranges(K, splits)
    assert sp == len(ranges)
    slab = sentinel_slab(M * N, sp)
    L.cdm_gemm_tn_f32(P(a), lda, M, K, P(b), ldb, N, splits, P(slab), _s())
    got = slab_parts(slab, sp, M, N, f"gemm_tn {name}")
    parts = R.gemm_tn_parts(c["a"], c["b"], splits)
    mags = R.gemm_tn_parts(np.abs(c["a"]), np.abs(c["b"]), splits)
    for z, (k0, k1) in enumerate(ranges):
        hold(got[z], parts[z], mags[z], data, "f32", k1 - k0 + 2, f"gemm_tn {name} split {z}")
    out = outbuf(M, N, N + 4, 0)
    L.cdm_slab_reduce(P(slab), sp, M, N, P(out), N + 4, 0, 1, N, 0, 1.0, _s())
    hold(take(out, (M, N), 0), parts.sum(0), mags.sum(0), data, "f32", K + sp + 2, f"gemm_tn {name} folded")


@pytest.mark.parametrize("case", R.TN_CASES, ids=lambda c: c[0])
def test_gemm_tn_f32(L, case):
    """cdm_gemm_tn_f32 (A^T B) at lda = M + 4, ldb = N + 4: K below a tile and not a multiple of 4; split K with M and
    N tails, every slab against its partial"""
    run_gemm_tn(L, case, "exact")


def test_gemm_tn_f32_gauss(L):
    run_gemm_tn(L, R.TN_GAUSS, "gauss")


@pytest.mark.parametrize("shape", [(10, 5, 12), (8, 5, 10)], ids=["m10", "n10"])
def test_gemm_tn_f32_rejects(L, shape):
    run_gemm_tn(L, ("R0", shape, 1), "exact", reject=True)


# ----------------------------------------------------------------------------------------------------------------
# slab reduce
# ----------------------------------------------------------------------------------------------------------------
def run_reduce(L, M, N, splits, data, perms=None, combos=None):
    c = R.reduce_case(M, N, splits, data)
    slab = T(c["slab"])
    mag = np.abs(c["slab"]).sum(0)
    for pname, s_m, s_hi, s_lo, cs, size in perms or R.reduce_perms(M, N):
        old = c["old"][:size]
        idx = R.slab_index(M, N, s_m, s_hi, s_lo, cs)
        for accumulate, scale in combos or [(a, s) for a in (0, 1) for s in R.SCALES]:
            what = f"slab_reduce {M}x{N} splits {splits} {pname} accumulate {accumulate} scale {scale}"
            out = T(np.concatenate([old, np.full(8, SENT)]))
            L.cdm_slab_reduce(P(slab), splits, M, N, P(out), s_m, s_hi, s_lo, cs, accumulate, scale, _s())
            got = Hh(out)
            assert (got[-8:] == SENT).all(), what + ": wrote past the end"
            ref = R.slab_reduce(c["slab"], old, s_m, s_hi, s_lo, cs, accumulate, scale)
            if data == "exact":
                exact(got[:-8], ref, what)
            else:
                bound = np.zeros(size)
                bound[idx] = chain_bound(splits, mag * abs(scale) + (np.abs(old[idx]) if accumulate else 0.0))
                check(got[:-8], ref, bound, what)


@pytest.mark.parametrize("splits", R.REDUCE_SPLITS)
@pytest.mark.parametrize("M,N", R.REDUCE_SHAPES)
def test_slab_reduce(L, M, N, splits):
    """cdm_slab_reduce itself: the scalar kernel (splits < 8, or N = 6) and the float4 kernel (its last block partly
    empty at (5, 36) and (3, 8)), every permutation the engine uses (identity, csplit = 0, the OIHW, ConvT and up0
    repacks) and one with s_m > N inside old values that must survive, accumulate 0 / 1, scale 1 / 0.5 / -2: per
    element equal to the reference, elements no (m, n) maps to unchanged"""
    run_reduce(L, M, N, splits, "exact")


@pytest.mark.parametrize("splits", [7, 17])
def test_slab_reduce_gauss(L, splits):
    run_reduce(L, 16, 132, splits, "gauss", combos=[(1, 0.5), (0, -2.0)])
