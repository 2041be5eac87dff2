"""ContextUnet forward / backward on the HIP kernels (explicit graph, no autograd inside).

Mirrors ContextUnet.forward (ContextUnet.py:42-60, == code/train_diffusion.py:48-66) block by block:

    init_conv (ResidualConvBlock is_res, random 1x1 shortcut)   diffusion_utilities.py:13-65
    down1/down2 (2x RCB + MaxPool2d(2))                          diffusion_utilities.py:103-116
    to_vec (AvgPool2d(h/4) + GELU)                               ContextUnet.py:17
    4x EmbedFC                                                    diffusion_utilities.py:118-145
    up0 (ConvTranspose2d k=h/4 on 1x1, GroupNorm(8), ReLU)       ContextUnet.py:26-30
    FiLM cemb*u + temb, up1/up2 (cat, ConvT 2x2, 2x RCB)         ContextUnet.py:57-58, diffusion_utilities.py:79-100
    out (conv3x3, GroupNorm(8), ReLU, conv3x3 -> 1)              ContextUnet.py:35-40

Memory layout: every activation is NHWC fp32 in HBM.  The three torch.cat calls are eliminated by
giving each concatenation a single buffer whose channel slices are written by their producers:

    catO  [B, H,   H,   2nf] = [ up2 output | init_conv output x0 ]
    catU2 [B, H/2, H/2, 2nf] = [ FiLM2(up1 output) | d1 = down1 output ]
    catU1 [B, H/4, H/4, 4nf] = [ FiLM1(up0 output) | d2 = down2 output ]

Train mode keeps every BatchNorm's pre-norm conv output y (the normalised/ReLU'd activation z is
kept only where the next conv reads it); the backward recomputes relu masks / max-pool argmaxes /
x-hat from y.  Eval mode folds BatchNorm into the conv weights and runs ReLU in the conv epilogue.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import torch

from ._lib import Mlp4, MlpDesc, lib

BN_EPS = 1e-5
BN_MOM = 0.1
GN_EPS = 1e-5
GN_GROUPS = 8
CHUNK = 128           # pixels per statistics partial (== GEMM M tile)
WGRAD_BLOCKS = 768    # grid of the kernel-row weight gradient: three whole rounds of 256 CUs (wgrad_splits)
EPI_RELU, EPI_ACCUM = 1, 2
APPLY_POOL, APPLY_FILM, APPLY_RESID, APPLY_RELU = 1, 2, 4, 8


def _p(t: Optional[torch.Tensor], off: int = 0):
    return None if t is None else t.data_ptr() + 4 * off


class Act:
    """NHWC activation view: channels [off, off+C) of a buffer whose pixel stride is ``ld`` floats."""
    __slots__ = ("buf", "C", "ld", "off")

    def __init__(self, buf: torch.Tensor, C: int, ld: Optional[int] = None, off: int = 0):
        self.buf, self.C, self.ld, self.off = buf, C, (C if ld is None else ld), off

    @property
    def p(self):
        return self.buf.data_ptr() + 4 * self.off

    def sl(self, c0: int, C: int) -> "Act":
        return Act(self.buf, C, self.ld, self.off + c0)


def _cdiv(a, b):
    return (a + b - 1) // b


class LayerSpec:
    """One Conv3x3 -> BatchNorm2d -> ReLU (diffusion_utilities.py:26-37) and its place in the U-Net's conv chain.

    kind: where its activation goes — "dense": a private z that the next layer reads; "resid" / "pool" / "film" /
    "plain": through that transform into a slice of a concatenation buffer.  src / dst name workspace buffers as
    (buffer, first channel, channels), the channels in units of n_feat; None is the z between two consecutive layers
    (for layer 0 the image).  The gradient of a cat* slice is the same slice of dcat*.
    src_slot / dst_slot: amax-slot keys of the two operands (h3).  Producers writing slices of one concatenation
    buffer share that buffer's slot (its consumers read the whole buffer, or a slice whose max the shared slot bounds
    from above — harmless for the scale).
    stage: the backward's on_stage name; STAGE_PROBE maps it to the forward's stage_probe point."""

    def __init__(self, index, name, cin, cout, S, stage, kind, src, dst):
        self.index, self.name, self.cin, self.cout, self.S = index, name, cin, cout, S
        self.stage, self.kind, self.src, self.dst = stage, kind, src, dst
        self.prev = self.next = None
        self.src_slot = src[0] if src else None          # None src: the previous layer's dst_slot (conv_layers)
        self.dst_slot = dst[0] if dst else "z:" + name
        self.w, self.b = name + ".0.weight", name + ".0.bias"
        self.bn = name + ".1"
        self.kc = conv_kc(cin, cout)


class ConvTSpec:
    """One ConvTranspose2d(cin, n_feat, 2, 2) (diffusion_utilities.py:86): reads the whole concatenation buffer `src`
    (Hin x Hin), writes `dst`; `consumer` is the conv layer that reads dst, so its dgrad writes the gradient of dst (and
    records its max in the slot g_slot for the h3 ConvT backward).  src and dst are their own amax-slot keys."""

    def __init__(self, name, stage, src, cin, Hin, dst, consumer):
        self.name, self.stage, self.src, self.cin, self.Hin, self.dst = name, stage, src, cin, Hin, dst
        self.consumer, self.g_slot = consumer, "gT:" + consumer.name


STAGE_PROBE = {"init": "x0", "down1": "d1", "down2": "d2", "up1": "film2", "up2": "u3"}


def conv_kc(cin: int, cout: int) -> int:
    """K order of a conv's packed weights: channel-chunk-major (16) when both channel counts allow."""
    return 16 if (cin % 16 == 0 and cout % 16 == 0) else 0


def conv_layers(nf: int, H: int, cin0: int = 1):
    """The 18 Conv3x3 -> BatchNorm -> ReLU layers in forward order, with the whole wiring of the U-Net's conv chain
    (LayerSpec); cin0 = the image channels the init conv reads (in_channels, padded to a multiple of 4 when > 1)."""
    L = []

    def rcb(stage, prefix, cin, cout, S, src=None, kind="dense", dst=None):
        L.append(LayerSpec(len(L), prefix + ".conv1", cin, cout, S, stage, "dense", src, None))
        L.append(LayerSpec(len(L), prefix + ".conv2", cout, cout, S, stage, kind, None, dst))

    rcb("init", "init_conv", cin0, nf, H, kind="resid", dst=("catO", 1, 1))
    rcb("down1", "down1.model.0", nf, nf, H, src=("catO", 1, 1))
    rcb("down1", "down1.model.1", nf, nf, H, kind="pool", dst=("catU2", 1, 1))
    rcb("down2", "down2.model.0", nf, 2 * nf, H // 2, src=("catU2", 1, 1))
    rcb("down2", "down2.model.1", 2 * nf, 2 * nf, H // 2, kind="pool", dst=("catU1", 2, 2))
    rcb("up1", "up1.model.1", nf, nf, H // 2, src=("yT1", 0, 1))
    rcb("up1", "up1.model.2", nf, nf, H // 2, kind="film", dst=("catU2", 0, 1))
    rcb("up2", "up2.model.1", nf, nf, H, src=("yT2", 0, 1))
    rcb("up2", "up2.model.2", nf, nf, H, kind="plain", dst=("catO", 0, 1))
    for a, b in zip(L, L[1:]):
        a.next, b.prev = b, a
        if b.src is None:
            b.src_slot = a.dst_slot
    return L


def convT_layers(nf: int, H: int, L):
    """The two 2x2 ConvT layers in forward order (L = conv_layers(...): each one's consumer)."""
    reads = {l.src[0]: l for l in L if l.src}
    return [ConvTSpec("up1.model.0", "up1", "catU1", 4 * nf, H // 4, "yT1", reads["yT1"]),
            ConvTSpec("up2.model.0", "up2", "catU2", 2 * nf, H // 2, "yT2", reads["yT2"])]


# 3x3 conv arithmetic: "fp32" = fp32 MFMA (v_mfma_f32_32x32x2_f32); "x6" = fp32-accurate split-bf16
# (6 cross terms on v_mfma_f32_32x32x16_bf16, see csrc/gemm_f32.hip); "h3" = fp32-class scaled fp16
# hi/lo split (3 cross terms on v_mfma_f32_32x32x16_f16; per-tensor power-of-two scale from max|.|);
# "x3" / "bf16" = reduced-precision variants (bf16x3 / plain bf16 operands, fp32 accumulate) for the
# mixed-precision configuration.
CONV_MATH = {"fp32": 0, "x6": 6, "x3": 3, "bf16": 1, "h3": 4}
NT_H3 = 4

MLPS = ("contextembed1", "timeembed1", "contextembed2", "timeembed2")


class UNetEngine:
    """Kernel-level ContextUnet for one (n_feat, n_cfeat, height) on one device."""

    def __init__(self, n_feat: int, n_cfeat: int, height: int, device, conv_math: str = "fp32", in_channels: int = 1):
        # the reference needs height % 4 == 0 (two MaxPool2d(2), AvgPool2d(h/4), ConvTranspose2d(k = h/4):
        # ContextUnet.py:17,27); the LDS-halo / band / fused paths take the map widths they support and every other
        # width runs the generic kernels (round 5: heights 20, 36, 48 tested)
        if n_feat % 8 or height % 4 or height < 4:
            raise ValueError("HIP path needs n_feat % 8 == 0 and height % 4 == 0")
        if conv_math not in CONV_MATH:
            raise ValueError(f"conv_math must be one of {sorted(CONV_MATH)}")
        self.nf, self.ncf, self.H = n_feat, n_cfeat, height
        # image channels (ContextUnet.py:6,14,39).  The reference's call sites all build in_channels = 1, for which the
        # C_in = 1 init-conv kernels and the C_out = 1 out.3 kernels run.  More channels run the general conv kernels
        # on NHWC images padded to cp = a multiple of 4 channels (zero image channels, zero weight columns / rows)
        if in_channels < 1:
            raise ValueError("in_channels must be >= 1")
        self.cimg = in_channels
        self.cp = 1 if in_channels == 1 else _cdiv(in_channels, 4) * 4
        self.conv_math = conv_math
        self.nterm = CONV_MATH[conv_math]
        # the 16-bit-MFMA kernel family with every train-mode fusion: h3 (fp32-class) and bf16 (C4 mixed precision)
        self.x16 = self.nterm in (1, NT_H3)
        self.h3 = self.nterm == NT_H3
        # BatchNorm backward fused into the staging of the layer's dgrad, which also stores the dy it computes for the
        # weight gradient (staged there instead of evaluated again in each of its 3 kernel-row blocks).  Under one-term
        # (bf16) arithmetic dy comes from an elementwise pass of its own (cdm_bn_bwd_dy) and the dgrad runs on the
        # forward's staging schedule (halo two chunks ahead), for which the BN-backward staging has no room.  The A/B
        # results that decided both forms: DESIGN.md section 3.3.  $CDM_FUSE_BN_BWD=0 keeps the separate apply kernel
        # (A/B checks)
        self.fuse_bn_bwd = self.x16 and os.environ.get("CDM_FUSE_BN_BWD", "1") != "0"
        # a dense BatchNorm + ReLU applied inside the next conv's staging ($CDM_FUSE_BN_FWD=0: apply kernel)
        self.fuse_bn_fwd = self.x16 and os.environ.get("CDM_FUSE_BN_FWD", "1") != "0"
        # a fused producer's BN-backward channel sums accumulated in its consumer's weight-gradient X staging (which
        # stages the producer's y anyway), after the consumer's dgrad wrote the producer's g: no separate pass over g and
        # y; the weight gradient stages a stored dy, so the sums fit (250 VGPRs, no spill): same-box A/B, 2 runs each,
        # C2 50.36-50.38 -> 49.39-49.45 ms per step (profiles/r4_ab_sums_dy_pass.txt).  $CDM_FUSE_BN_SUMS=0: off
        self.fuse_bn_sums = self.x16 and os.environ.get("CDM_FUSE_BN_SUMS", "1") == "1"
        # C4 mixed precision (bf16 arithmetic, train mode): the fused Conv -> BN -> ReLU chain's pre-norm outputs y and
        # their gradients g are stored as bf16 (torch.autocast keeps conv outputs and their gradients in bf16), halving
        # the bytes every fused conv stages; BN statistics, accumulators, master weights stay fp32.  The chain's ends
        # (concatenation slices, pool / FiLM / residual outputs, the C_in = 1 init conv) stay fp32.
        # $CDM_ACT16=0 keeps fp32 activations (A/B checks).
        self.act16 = self.nterm == 1 and os.environ.get("CDM_ACT16", "1") != "0"
        # eval: the pool / FiLM / residual applies in the conv epilogue (fuses_eval)
        self.fuse_eval = self.x16 and os.environ.get("CDM_FUSE_EVAL", "1") != "0"
        self.device = torch.device(device)
        self.layers = conv_layers(n_feat, height, self.cp)
        self.convT = convT_layers(n_feat, height, self.layers)
        self.stages = {st: [l for l in self.layers if l.stage == st] for st in STAGE_PROBE}
        self.KK0 = (height // 4) ** 2
        # up0 on large maps (config 5: k = 64, 1.07 G weights): VALU kernels over the weights in their reference layout
        # (cdm_up0_fwd / cdm_up0_wgrad) and one W^T for the input gradient, instead of two 4.3 GB repacks per step
        self.up0_large = self.KK0 >= 1024 and self.KK0 % 256 == 0 and (2 * n_feat) % 16 == 0 and 2 * n_feat <= 512
        self.kc_out0 = conv_kc(2 * n_feat, n_feat)
        self.pk: Dict[str, torch.Tensor] = {}
        self._pk_key = None
        self.train_pack_token = None     # identity of the autograd forward whose train pack pk holds (model.py)
        self._ones =torch.ones(4 * n_feat, device=self.device)
        self._zeros = torch.zeros(4 * n_feat, device=self.device)
        self._amax = torch.zeros(2, device=self.device)     # h3: max|A|, max|B| of the current launch
        # h3 train: batched repack (3 launches per step); $CDM_BATCH_REPACK=0 keeps the per-layer launches (A/B)
        self.batch_repack = os.environ.get("CDM_BATCH_REPACK", "1") != "0"
        # measurement hook: probe(args) before every 3x3 conv launch, args = the _conv3x3 arguments (bench.py replays
        # the dominant conv's launches of a real train step on their real operands); None in production
        self.launch_probe = None
        # diagnostic hook: stage_probe(stage, ws) at fixed points of the forward ("x0", "d1", "d2", "emb", "film2", "u3";
        # tools/t1500_steps.py substitutes reference values there to locate an error source); None in production
        self.stage_probe = None
        self._batch_key = None

    # ------------------------------------------------------------------------------------------
    # weight packing (OIHW / [Cin][Cout][kh][kw] -> GEMM layouts; eval: BatchNorm folded)
    # ------------------------------------------------------------------------------------------
    def _repack_h3_train_batched(self, P, stream: int):
        """h3 / bf16 train mode: every 3x3 conv with C_in > 1 (and out.0) repacked in 3 launches — clear the max|W|
        slots, max|W| per layer, the split images straight from OIHW (cdm_pack_split_conv3x3_batch; bf16: the one-term
        hi plane, round 5 — it replaced 40 split + 18 pack launches per C4 step)."""
        nf = self.nf
        specs = [(l.name, self._layer_w(P, l), l.cin, l.cout, l.kc) for l in self.layers if l.cin > 1]
        specs.append(("out.0", P["out.0.weight"], 2 * nf, nf, self.kc_out0))
        key = tuple(w.data_ptr() for _, w, *_ in specs)
        if self._batch_key != key:
            import ctypes

            class Job(ctypes.Structure):
                _fields_ = [("W", ctypes.c_void_p), ("Cin", ctypes.c_int), ("Cout", ctypes.c_int), ("kc", ctypes.c_int),
                            ("pad", ctypes.c_int), ("wpk_x", ctypes.c_void_p), ("wdg_x", ctypes.c_void_p),
                            ("amax", ctypes.c_void_p)]
            assert ctypes.sizeof(Job) == 48
            slots = torch.zeros(len(specs), device=self.device)
            arr = (Job * len(specs))()
            for i, (name, W, cin, cout, kc) in enumerate(specs):
                wx = self._buf(name + ".wpk_x", (_cdiv(9 * cin, 16) * 3 * cout * 16,), torch.bfloat16)
                wdx = self._buf(name + ".wdg_x", (_cdiv(9 * cout, 16) * 3 * cin * 16,), torch.bfloat16)
                self.pk[name + ".wpk_x"], self.pk[name + ".wdg_x"] = wx, wdx
                self.pk[name + ".wpk_amax"] = self.pk[name + ".wdg_amax"] = slots[i:i + 1]
                arr[i] = Job(W.data_ptr(), cin, cout, kc, 0 if self.h3 else 1, wx.data_ptr(), wdx.data_ptr(),
                             slots.data_ptr() + 4 * i)
            raw = bytes(memoryview(arr).cast("B"))
            self._batch_jobs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
            self._batch_slots, self._batch_n = slots, len(specs)
            self._batch_max = max(cin * cout * 9 for _, _, cin, cout, _ in specs)
            self._batch_key = key
        lb = lib()
        lb.cdm_zero_f32(_p(self._batch_slots), self._batch_n, stream)
        lb.cdm_pack_split_conv3x3_batch(_p(self._batch_jobs), self._batch_n, self._batch_max, stream)

    def repack(self, P: Dict[str, torch.Tensor], train: bool, stream: int, key=None):
        if key is not None and self._pk_key == (key, train):
            return
        self.train_pack_token = None          # the pack changes owner (model.py re-packs before a stale backward)
        lb = lib(); nf = self.nf
        batched = train and self.x16 and self.batch_repack
        if batched:
            self._repack_h3_train_batched(P, stream)
        for l in self.layers:
            if batched and l.cin > 1:
                continue
            W, b = self._layer_w(P, l), P[l.b]
            if train:
                wpk = self._buf(l.name + ".wpk", (9 * l.cin, l.cout))
                wdg = (self._buf(l.name + ".wdg", (9 * l.cout, l.cin))) if l.cin > 1 else None
                lb.cdm_pack_conv3x3(_p(W), _p(b), l.cin, l.cout, None, None, None, None, 0.0, _p(wpk), None,
                                    _p(wdg), l.kc, stream)
                self.pk[l.name + ".wpk"] = wpk
                if wdg is not None:
                    self.pk[l.name + ".wdg"] = wdg
                    self._split(l.name + ".wpk", 9 * l.cin, l.cout, stream)
                    self._split(l.name + ".wdg", 9 * l.cout, l.cin, stream)
            else:
                wpk = self._buf(l.name + ".wpk_e", (9 * l.cin, l.cout))
                bpk = self._buf(l.name + ".bpk_e", (l.cout))
                bn = l.bn
                lb.cdm_pack_conv3x3(_p(W), _p(b), l.cin, l.cout, _p(P[bn + ".weight"]), _p(P[bn + ".bias"]),
                                    _p(P[bn + ".running_mean"]), _p(P[bn + ".running_var"]), BN_EPS, _p(wpk),
                                    _p(bpk), None, l.kc, stream)
                self.pk[l.name + ".wpk_e"] = wpk
                self.pk[l.name + ".bpk_e"] = bpk
                if l.cin > 1:
                    self._split(l.name + ".wpk_e", 9 * l.cin, l.cout, stream)
        # out.0 (GroupNorm follows: never folded)
        if not batched:
            wpk = self._buf("out.0.wpk", (9 * 2 * nf, nf))
            wdg = self._buf("out.0.wdg", (9 * nf, 2 * nf))
            lb.cdm_pack_conv3x3(_p(P["out.0.weight"]), _p(P["out.0.bias"]), 2 * nf, nf, None, None, None, None, 0.0,
                                _p(wpk), None, _p(wdg) if train else None, self.kc_out0, stream)
            self.pk["out.0.wpk"], self.pk["out.0.wdg"] = wpk, wdg
            self._split("out.0.wpk", 9 * 2 * nf, nf, stream)
            if train:
                self._split("out.0.wdg", 9 * nf, 2 * nf, stream)
        if self.cp > 1:
            # out.3 (n_feat -> in_channels) on the general conv kernels: weights / bias padded to cp output channels
            cp, C = self.cp, self.cimg
            w3 = self._buf("out.3.wpad", (cp, nf, 3, 3))
            b3 = self._buf("out.3.bpad", (cp,))
            w3[C:].zero_(); w3[:C].copy_(P["out.3.weight"])
            b3[C:].zero_(); b3[:C].copy_(P["out.3.bias"])
            self.pk["out.3.wpad"], self.pk["out.3.bpad"] = w3, b3
            wpk = self._buf("out.3.wpk", (9 * nf, cp))
            wdg = self._buf("out.3.wdg", (9 * cp, nf))
            lb.cdm_pack_conv3x3(_p(w3), _p(b3), nf, cp, None, None, None, None, 0.0, _p(wpk), None,
                                _p(wdg) if train else None, conv_kc(nf, cp), stream)
            self.pk["out.3.wpk"], self.pk["out.3.wdg"] = wpk, wdg
            self._split("out.3.wpk", 9 * nf, cp, stream)
            if train:
                self._split("out.3.wdg", 9 * cp, nf, stream)
        for name, cin in (("up1.model.0", 4 * nf), ("up2.model.0", 2 * nf)):
            wt = self._buf(name + ".wt", (cin, 4 * nf))
            wtT = self._buf(name + ".wtT", (4 * nf, cin))
            lb.cdm_pack_convT(_p(P[name + ".weight"]), cin, nf, 4, _p(wt), _p(wtT) if train else None, stream)
            self.pk[name + ".wt"], self.pk[name + ".wtT"] = wt, wtT
            if self.x16:
                self._split(name + ".wt", cin, 4 * nf, stream)
                if train:
                    self._split(name + ".wtT", 4 * nf, cin, stream)
        c0 = 2 * nf
        if self.up0_large:
            pass   # W[ci][(co, ij)] is used in place (B > 16 input gradients build their W^T in the backward)
        else:
            w0 = self._buf("up0.wt", (c0, self.KK0 * c0))
            w0T = self._buf("up0.wtT", (self.KK0 * c0, c0))
            lb.cdm_pack_convT(_p(P["up0.0.weight"]), c0, c0, self.KK0, _p(w0), _p(w0T) if train else None, stream)
            self.pk["up0.wt"], self.pk["up0.wtT"] = w0, w0T
            if self.x16:    # the forward GEMM on the 16-bit matrix cores (cdm_gemm_x16)
                self._split("up0.wt", c0, self.KK0 * c0, stream)
        for m in MLPS:
            w2 = P[m + ".model.2.weight"]
            E = w2.shape[0]
            w2t = self._buf(m + ".w2t", (E, E))
            lb.cdm_transpose(_p(w2), E, E, _p(w2t), stream)
            self.pk[m + ".w2t"] = w2t
        self._pk_key = (key, train) if key is not None else None

    def _layer_w(self, P, l: "LayerSpec") -> torch.Tensor:
        """Conv l's OIHW weights; the init conv's with zero columns for the padded image channels (in_channels > 1)."""
        W = P[l.w]
        if l is not self.layers[0] or self.cp == self.cimg:
            return W
        wp = self.pk["init.wpad"] = self._buf("init.wpad", (self.nf, self.cp, 3, 3))
        wp[:, self.cimg:].zero_()
        wp[:, :self.cimg].copy_(W)
        return wp

    def invalidate(self):
        """Parameters changed behind torch's version counters (fused Adam): drop the cached eval pack."""
        self._pk_key = None

    def _buf(self, name, shape, dtype=torch.float32):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        t = self.pk.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(*shape, device=self.device, dtype=dtype)
        return t

    def _split(self, name, K, N, stream):
        """16-bit split of the packed fp32 [K][N] weights pk[name] -> pk[name + "_x"] (bf16 hi/mid/lo, or
        for h3 the scaled fp16 hi/lo with max|W| in pk[name + "_amax"])."""
        if not self.nterm:
            return
        xb = self._buf(name + "_x", (_cdiv(K, 16) * 3 * N * 16,), torch.bfloat16)
        if self.nterm == NT_H3:
            am = self._buf(name + "_amax", (1,))
            lib().cdm_amax_f32(_p(self.pk[name]), K, N, N, _p(am), 0, stream)
            lib().cdm_split_f16x2(_p(self.pk[name]), N, K, N, _p(am), _p(xb), stream)
            self.pk[name + "_amax"] = am
        else:
            lib().cdm_split_bf16x3(_p(self.pk[name]), N, K, N, _p(xb), stream)
        self.pk[name + "_x"] = xb

    def _wamax(self, key):
        """Device max|W| of the split weights pk[key + "_x"] (h3 scale), None for the other arithmetics."""
        return _p(self.pk[key + "_amax"]) if self.h3 else None

    def conv3x3(self, key, x_p, B, S, cin, ldx, bias_p, y_p, ldy, cout, flags, stats_p, stats_ld, kc, s,
                amax_x=None, amax_y=None, pre=None, ymm=None, dt=0):
        """3x3 conv (fwd or dgrad) with the packed weights pk[key], in this engine's conv arithmetic.

        h3 only: amax_x = device max|x| written by x's producer (None: measured here by a separate pass);
        amax_y = slot that receives max|y| for the next conv; pre = (scale, shift) pointers: the input is
        relu(x * scale + shift) of the previous layer's pre-norm output, applied while staging; ymm = (ptr, ld):
        per-channel max / min keys of y for the next layer's fused apply."""
        args = (key, x_p, B, S, cin, ldx, bias_p, y_p, ldy, cout, flags, stats_p, stats_ld, kc, s, amax_x, amax_y,
                pre, ymm, dt)
        if self.launch_probe is not None:
            self.launch_probe(args)
        self._conv3x3(*args)

    def _conv3x3(self, key, x_p, B, S, cin, ldx, bias_p, y_p, ldy, cout, flags, stats_p, stats_ld, kc, s, amax_x,
                 amax_y, pre, ymm, dt=0):
        """dt (bf16 activations, C4): bit 0 the source holds bf16, bit 1 the output is stored as bf16."""
        if self.x16:
            if self.h3 and amax_x is None:
                assert pre is None
                amax_x = _p(self._amax)
                lib().cdm_amax_f32(x_p, B * S * S, cin, ldx, amax_x, 0, s)
            if pre is not None or ymm is not None:
                ps, pt = pre if pre is not None else (None, None)
                ym, yld = ymm if ymm is not None else (None, 0)
                lib().cdm_conv3x3_fwd_x16_ex(x_p, B, S, S, cin, ldx, ps, pt, _p(self.pk[key + "_x"]), amax_x,
                                             self._wamax(key), bias_p, y_p, ldy, cout, flags, stats_p, stats_ld, kc,
                                             amax_y, ym, yld, self.nterm, dt, s)
                return
            lib().cdm_conv3x3_fwd_x16(x_p, B, S, S, cin, ldx, _p(self.pk[key + "_x"]), amax_x, self._wamax(key),
                                      bias_p, y_p, ldy, cout, flags, stats_p, stats_ld, kc, amax_y, self.nterm, dt, s)
        elif self.nterm:
            lib().cdm_conv3x3_fwd_x3(x_p, B, S, S, cin, ldx, _p(self.pk[key + "_x"]), bias_p, y_p, ldy, cout, flags,
                                     stats_p, stats_ld, kc, self.nterm, s)
        else:
            lib().cdm_conv3x3_fwd(x_p, B, S, S, cin, ldx, _p(self.pk[key]), bias_p, y_p, ldy, cout, flags, stats_p,
                                  stats_ld, kc, s)

    def halo_addressable(self, B: int, S: int) -> bool:
        """The LDS-halo conv addresses its sources by 32-bit byte offsets: B*S*S pixels x the widest row of any
        activation / gradient buffer at that resolution (2 n_feat floats; 4 n_feat at H/4, catU1) must stay below
        4 GiB for the fused (halo-only) paths."""
        ld = (4 if S == self.H // 4 else 2) * self.nf
        return B * S * S * ld * 4 < 2 ** 32

    def fuses_bn_fwd(self, l: "LayerSpec", kind: str, B: int = 1) -> bool:
        """Producer l's train-mode BatchNorm apply (z = relu(y s + t)) runs inside the staging of the next conv (its
        forward and its weight gradient): z is never written.  Needs the LDS-halo path for both convs (max / min
        epilogue on l, BN-ReLU staging on the consumer) and the kernel-row weight gradient for the consumer."""
        c = l.next
        if not (self.fuse_bn_fwd and kind == "dense" and self.halo_addressable(B, l.S)) or c is None:
            return False
        widths = (32, 64, 128, 256) if self.h3 else (32, 64)     # the wide-row LDS-halo conv is h3-only
        halo = lambda L: L.kc == 16 and L.S in widths and (L.S * L.S) % 256 == 0   # noqa: E731
        # the producer's max / min of y: from its conv epilogue (LDS-halo path), or from the statistics pass of the
        # C_in = 1 init conv (cdm_reduce_stats_mm)
        return ((l.cin == 1 or halo(l)) and halo(c) and c.cin == l.cout and c.cin <= 256 and c.cin % 128 == 0
                and c.cout % 128 == 0 and c.S == l.S)

    def fuses_gn_out(self) -> bool:
        """out.1's GroupNorm + ReLU runs inside out.3's kernels (forward; train: and its weight gradient): zO is never
        written, and its workspace buffer is not allocated."""
        nf, H = self.nf, self.H
        return self.cp == 1 and nf % 16 == 0 and H <= 256 and 256 % H == 0

    def fuses_bn_bwd(self, l: "LayerSpec", kind: str, B: int = 1) -> bool:
        """Layer l's BN backward runs inside its dgrad staging (cdm_conv3x3_dgrad_x16_bnbwd_dy), which hands dy to its
        weight gradient."""
        return (self.fuse_bn_bwd and kind in ("dense", "plain", "resid") and l.cin > 1 and l.index > 0
                and l.S in ((32, 64, 128) if self.h3 else (32, 64))
                and self.halo_addressable(B, l.S)
                and l.kc == 16 and l.cin % 128 == 0 and l.cout % 128 == 0 and l.cout <= 256)

    # h3 operand maxima: one device slot per producer, zeroed at the start of every forward --------------
    def _slot(self, ws, key):
        """Pointer to the amax slot `key` of this workspace, assigned on first use (None unless the arithmetic is h3;
        None for no key — the image of in_channels > 1 has none: its max is measured by the conv call)."""
        if self.nterm != NT_H3 or key is None:
            return None
        i = ws.aslot.get(key)
        if i is None:
            i = ws.aslot[key] = len(ws.aslot)
            assert i < ws.amax.numel()
        return _p(ws.amax) + 4 * i

    # ------------------------------------------------------------------------------------------
    def workspace(self, B: int, train: bool, frozen: bool = False) -> "Workspace":
        """frozen: a train-structured workspace for the forward / backward of model.eval() under autograd (BatchNorm on
        the running statistics); it keeps fp32 activations under C4's bf16 arithmetic, like the no-grad eval path, so an
        eval model returns the same eps whether or not autograd records it."""
        return Workspace(self, B, train, frozen)

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def forward(self, ws: "Workspace", P, x: torch.Tensor, t_in: torch.Tensor, c_in: Optional[torch.Tensor],
                sc_w: torch.Tensor, sc_b: torch.Tensor, sc_split: int, stream: int, out: Optional[torch.Tensor] = None,
                frozen: bool = False):
        """x [B,H,W] fp32 (C=1, NCHW == NHWC; in_channels > 1: NHWC [B*H*W, cp] with zero padding channels), t_in [rows_t]
        (rows 1 or B), c_in [rows_c, ncf] or None (zeros).

        sc_w/sc_b: shortcut 1x1 conv weights, [2, nf] when sc_split < B (CFG halves) else [nf]-shaped.
        frozen (train-mode workspace only): BatchNorm with the running statistics, not updated — the forward of
        model.eval() kept for a backward (backward(..., frozen=True)).
        Returns eps [B, H, W] (in_channels > 1: NHWC [B*H*W, cp]; written into ``out`` when given)."""
        lb = lib(); s = stream
        nf, H, B = self.nf, self.H, ws.B
        H2 = H // 4
        train = ws.train
        assert train or not frozen
        assert not (frozen and ws.act16), "eval-mode forwards keep fp32 activations: use workspace(B, True, frozen=True)"
        ws.frozen = frozen
        eps = out if out is not None else ws.eps
        ws.x_in = x
        if self.cp > 1:
            assert x.numel() == B * H * H * self.cp
            ws.plan[0].src = Act(x, self.cp)
        ws.sc_pending = (sc_w, sc_b, sc_split)
        if self.nterm == NT_H3:
            lb.cdm_zero_f32(_p(ws.amax), ws.amax.numel(), s)
        if train and ws.fused_fwd and self.h3:
            half = ws.ymm.numel() // 2
            lb.cdm_fill_i32(_p(ws.ymm), half, -2 ** 31, s)               # max keys
            lb.cdm_fill_i32(_p(ws.ymm) + 4 * half, half, 2 ** 31 - 1, s)  # min keys
        # ---------------- encoder ----------------
        probe = self.stage_probe or (lambda stage, ws_: None)
        for stage in ("init", "down1", "down2"):
            self._stage_fwd(ws, P, stage, s, x)
        # ---------------- to_vec ----------------
        d2 = ws.catU1.sl(2 * nf, 2 * nf)
        lb.cdm_reduce_sum(d2.p, d2.ld, B, H2 * H2, 2 * nf, H2 * H2, _p(ws.hsum), s)
        lb.cdm_avgpool_gelu_fin(_p(ws.hsum), B, 2 * nf, H2 * H2, _p(ws.hpre), _p(ws.hv), s)
        # ---------------- embeddings ----------------
        rows_t = t_in.numel()
        if c_in is None:
            c_in = ws.c_zero
        rows_c = c_in.shape[0]
        ws.t_rows, ws.c_rows = rows_t, rows_c
        ws.t_x, ws.c_x = t_in, c_in
        d = Mlp4()
        for k, m in enumerate(MLPS):
            is_t = m.startswith("time")
            E = (2 if m.endswith("1") else 1) * nf
            md = d.m[k]
            md.x = _p(t_in if is_t else c_in); md.rows = rows_t if is_t else rows_c
            md.in_dim = 1 if is_t else self.ncf; md.E = E
            md.w1 = _p(P[m + ".model.0.weight"]); md.b1 = _p(P[m + ".model.0.bias"])
            md.w2 = _p(P[m + ".model.2.weight"]); md.w2t = _p(self.pk[m + ".w2t"]); md.b2 = _p(P[m + ".model.2.bias"])
            md.pre = _p(ws.emb_pre[m]) if train else None
            md.h = _p(ws.emb_h[m]) if train else None
            md.out = _p(ws.emb[m])
        lb.cdm_embed_fwd(ctypes_addr(d), s)
        ws._mlp = d
        probe("emb", ws)
        # ---------------- up0: ConvT(k=h/4) on the 1x1 map, GroupNorm(8), ReLU, FiLM1 -> catU1[:, :2nf] ----
        c0 = 2 * nf
        if self.up0_large:
            lb.cdm_up0_fwd(_p(ws.hv), B, c0, _p(P["up0.0.weight"]), self.KK0, _p(P["up0.0.bias"]), _p(ws.y0), s)
        elif self.x16:
            # round 5: h3 / bf16 on the matrix cores (the fp32 MFMA GEMM took 105 us per sampling step at B = 256)
            am_hv = None
            if self.h3:
                am_hv = _p(self._amax)
                lb.cdm_amax_f32(_p(ws.hv), B, c0, c0, am_hv, 0, s)
            lb.cdm_gemm_x16(_p(ws.hv), c0, B, c0, _p(self.pk["up0.wt_x"]), am_hv, self._wamax("up0.wt"),
                            self.KK0 * c0, _p(ws.y0), self.KK0 * c0, _p(P["up0.0.bias"]), c0, None, self.nterm, s)
        else:
            lb.cdm_gemm_f32(_p(ws.hv), c0, B, c0, _p(self.pk["up0.wt"]), self.KK0 * c0, self.KK0 * c0, _p(ws.y0),
                            self.KK0 * c0, _p(P["up0.0.bias"]), c0, 0, 1, None, s)
        self._gn_fwd(ws, P, "up0.1", Act(ws.y0, c0), B, H2, c0, ws.gn0, stats_from_conv=False, stream=s)
        ce1, te1 = ws.emb["contextembed1"], ws.emb["timeembed1"]
        u1 = ws.catU1.sl(0, c0)
        lb.cdm_norm_apply_fwd(APPLY_FILM | APPLY_RELU, _p(ws.y0), c0, B, H2, H2, c0, _p(ws.gn0["scale"]),
                              _p(ws.gn0["shift"]), c0, _p(ce1), c0 if rows_c > 1 else 0, _p(te1),
                              c0 if rows_t > 1 else 0, None, None, None, 0, u1.p, u1.ld, self._slot(ws, "catU1"), s)
        # ---------------- up1, up2 ----------------
        for ct in self.convT:
            self.convT2x2(ws, ct, P, s)
            self._stage_fwd(ws, P, ct.stage, s, x)
        # ---------------- out ----------------
        self.conv3x3("out.0.wpk", ws.catO.p, B, H, 2 * nf, 2 * nf, _p(P["out.0.bias"]), _p(ws.yO), nf, nf, 0,
                     _p(ws.slab), nf, self.kc_out0, s, amax_x=self._slot(ws, "catO"))
        probe("yO", ws)
        # out.1's GroupNorm statistics come from out.0's epilogue partials (128-pixel tiles) when no tile spans two images
        self._gn_fwd(ws, P, "out.1", Act(ws.yO, nf), B, H, nf, ws.gnO, stats_from_conv=(H * H) % CHUNK == 0, stream=s)
        if self.fuses_gn_out():
            # out.1's GroupNorm + ReLU applied in out.3's staging (train: and in out.3's weight gradient): zO never
            # written
            lb.cdm_conv3x3_cout1_fwd_gn(_p(ws.yO), nf, B, H, H, nf, _p(ws.gnO["scale"]), _p(ws.gnO["shift"]),
                                        _p(P["out.3.weight"]), _p(P["out.3.bias"]), _p(eps), s)
            return eps
        zslot = self._slot(ws, "zO") if self.cp > 1 else None
        lb.cdm_norm_apply_fwd(APPLY_RELU, _p(ws.yO), nf, B, H, H, nf, _p(ws.gnO["scale"]), _p(ws.gnO["shift"]), nf,
                              None, 0, None, 0, None, None, None, 0, _p(ws.zO), nf, zslot, s)
        if self.cp > 1:   # out.3: n_feat -> in_channels (padded to cp) on the general conv kernels
            self.conv3x3("out.3.wpk", _p(ws.zO), B, H, nf, nf, _p(self.pk["out.3.bpad"]), _p(eps), self.cp, self.cp, 0,
                         None, 0, conv_kc(nf, self.cp), s, amax_x=zslot)
            return eps
        lb.cdm_conv3x3_cout1_fwd(_p(ws.zO), nf, B, H, H, nf, _p(P["out.3.weight"]), _p(P["out.3.bias"]), _p(eps), s)
        return eps

    def _stage_fwd(self, ws, P, stage, s, x):
        for l in self.stages[stage]:
            (self._conv_bn_train if ws.train else self._conv_bn_eval)(ws, ws.plan[l.index], P, s, x)
        if self.stage_probe is not None:
            self.stage_probe(STAGE_PROBE[stage], ws)

    def convT2x2(self, ws, ct: ConvTSpec, P, s):
        """ConvTranspose2d(cin, nf, 2, 2) (diffusion_utilities.py:86) of x [B,Hin,Hin,cin] into y [B,2Hin,2Hin,nf]."""
        nf, B, Hin, cin, name = self.nf, ws.B, ct.Hin, ct.cin, ct.name
        x, y = getattr(ws, ct.src), getattr(ws, ct.dst)
        if self.x16:
            lib().cdm_convT2x2_fwd_x16(x.p, B, Hin, Hin, cin, x.ld, _p(self.pk[name + ".wt_x"]),
                                       self._slot(ws, ct.src), self._wamax(name + ".wt"), _p(P[name + ".bias"]),
                                       _p(y), nf, nf, self._slot(ws, ct.dst), self.nterm, s)
        else:
            lib().cdm_convT2x2_fwd(x.p, B, Hin, Hin, cin, x.ld, _p(self.pk[name + ".wt"]), _p(P[name + ".bias"]),
                                   _p(y), nf, nf, self._slot(ws, ct.dst), s)

    def _conv_bn_train(self, ws, p: "LayerPlan", P, s, x):
        """Train forward of one layer: the conv with the statistics partials in its epilogue, the BatchNorm finalize,
        and the apply — unless the next conv's staging applies z = relu(y s + t) itself (p.fused_fwd)."""
        lb = lib()
        l, y, st = p.l, p.y, p.bn
        B, S = ws.B, l.S
        ymm_p, ymm_ld = p.ymm or (None, 0)
        if l.cin == 1:
            lb.cdm_conv3x3_cin1_fwd(_p(x), B, S, S, _p(self.pk[l.name + ".wpk"]), _p(P[l.b]), _p(y), l.cout,
                                    l.cout, 0, None, s)
            lb.cdm_reduce_stats_mm(_p(y), l.cout, B, S * S, l.cout, CHUNK, _p(ws.slab), ymm_p, ymm_ld, s)
            ntiles = B * _cdiv(S * S, CHUNK)
        else:
            yslot = self._slot(ws, "y:" + l.name) if p.fused else None
            self.conv3x3(l.name + ".wpk", p.src.p, B, S, l.cin, p.src.ld, _p(P[l.b]), _p(y), l.cout, l.cout, 0,
                         _p(ws.slab), l.cout, l.kc, s, amax_x=self._slot(ws, l.src_slot), amax_y=yslot, pre=p.pre,
                         ymm=p.ymm, dt=p.dt_fwd)
            ntiles = _cdiv(B * S * S, CHUNK)
        bn = l.bn
        nparts = fold(ws, _p(ws.slab), ntiles, 2, l.cout, s)
        zslot = self._slot(ws, l.dst_slot) if p.fused_fwd else None
        if ws.frozen:
            lb.cdm_bn_fwd_frozen(l.cout, _p(P[bn + ".weight"]), _p(P[bn + ".bias"]), _p(P[bn + ".running_mean"]),
                                 _p(P[bn + ".running_var"]), BN_EPS, _p(st["mean"]), _p(st["invstd"]),
                                 _p(st["scale"]), _p(st["shift"]), ymm_p, ymm_ld, zslot, s)
        else:
            lb.cdm_bn_fwd_finalize(_p(ws.dpart), nparts, 2, l.cout, float(B * S * S), _p(P[bn + ".weight"]),
                                   _p(P[bn + ".bias"]), _p(P[bn + ".running_mean"]), _p(P[bn + ".running_var"]),
                                   _p(P[bn + ".num_batches_tracked"]), BN_MOM, BN_EPS, _p(st["mean"]),
                                   _p(st["invstd"]), _p(st["scale"]), _p(st["shift"]), ymm_p, ymm_ld, zslot, s)
        if not p.fused_fwd:
            self._apply(ws, p, st["scale"], st["shift"], APPLY_RELU, x, s)

    def _conv_bn_eval(self, ws, p: "LayerPlan", P, s, x):
        """Eval forward of one layer: BatchNorm folded into the packed weights, ReLU in the conv's epilogue; a pool /
        FiLM / residual output transform in that epilogue too (fuses_eval), else by the apply kernel from y."""
        l = p.l
        B, S = ws.B, l.S
        dense = l.kind in ("dense", "plain")
        outp = p.dst if dense else Act(p.y, l.cout)
        dslot = self._slot(ws, l.dst_slot) if dense else None
        if l.cin == 1:
            lib().cdm_conv3x3_cin1_fwd(_p(x), B, S, S, _p(self.pk[l.name + ".wpk_e"]), _p(self.pk[l.name + ".bpk_e"]),
                                       outp.p, outp.ld, l.cout, 1, dslot, s)
        elif not dense and self.fuses_eval(l, B):
            self._conv_eval_fused(ws, p, x, s)       # y is never written
            return
        else:
            self.conv3x3(l.name + ".wpk_e", p.src.p, B, S, l.cin, p.src.ld, _p(self.pk[l.name + ".bpk_e"]), outp.p,
                         outp.ld, l.cout, EPI_RELU, None, 0, l.kc, s, amax_x=self._slot(ws, l.src_slot), amax_y=dslot)
        if not dense:
            self._apply(ws, p, self._ones, self._zeros, 0, x, s)

    def _transform_operands(self, ws, l: LayerSpec, x):
        """(sc_x, sc_w, sc_b, split), (film_a, film_a_ld, film_b, film_b_ld) of layer l's output transform: the image
        and the shortcut draws of a "resid" layer, the second embeddings of the "film" layer, null for the others."""
        if l.kind == "resid":
            sc_w, sc_b, split = ws.sc_pending
            return (_p(x), _p(sc_w), _p(sc_b), split), (None, 0, None, 0)
        if l.kind == "film":
            C = l.cout
            return (None, None, None, 0), (_p(ws.emb["contextembed2"]), C if ws.c_rows > 1 else 0,
                                           _p(ws.emb["timeembed2"]), C if ws.t_rows > 1 else 0)
        return (None, None, None, 0), (None, 0, None, 0)

    def _apply(self, ws, p: "LayerPlan", scale, shift, relu, x, s):
        """z = [relu](y scale + shift), through the layer's output transform, into its destination."""
        l, dst = p.l, p.dst
        B, S, C = ws.B, l.S, l.cout
        am = self._slot(ws, l.dst_slot)
        if l.kind == "resid" and self.cp > 1:
            sc_w, sc_b, split = ws.sc_pending
            lib().cdm_norm_apply_fwd_resid_c(relu, _p(p.y), C, B, S, S, C, _p(scale), _p(shift), _p(x), self.cp,
                                             self.cimg, _p(sc_w), _p(sc_b), split, dst.p, dst.ld, am, s)
            return
        resid, film = self._transform_operands(ws, l, x)
        flags = {"pool": APPLY_POOL, "film": APPLY_FILM, "resid": APPLY_RESID}.get(l.kind, 0) | relu
        lib().cdm_norm_apply_fwd(flags, _p(p.y), C, B, S, S, C, _p(scale), _p(shift), 0, *film, *resid, dst.p, dst.ld,
                                 am, s)

    def fuses_eval(self, l: "LayerSpec", B: int) -> bool:
        """Eval forward of a pool / FiLM / residual layer with its output transform in the LDS-halo conv's epilogue
        (cdm_conv3x3_fwd_x16_fused: 32^2 / 64^2 maps, 16-bit arithmetics); $CDM_FUSE_EVAL=0 keeps the apply kernel."""
        return (self.fuse_eval and l.cin > 1 and l.kc == 16 and l.S in (32, 64) and l.cout % 128 == 0
                and self.halo_addressable(B, l.S) and not (self.cp > 1 and l.kind == "resid"))

    def _conv_eval_fused(self, ws, p: "LayerPlan", x, s):
        lb = lib()
        l, src, dst = p.l, p.src, p.dst
        B, S = ws.B, l.S
        key = l.name + ".wpk_e"
        amax_x = self._slot(ws, l.src_slot)
        if self.h3 and amax_x is None:
            amax_x = _p(self._amax)
            lb.cdm_amax_f32(src.p, B * S * S, l.cin, src.ld, amax_x, 0, s)
        resid, film = self._transform_operands(ws, l, x)
        lb.cdm_conv3x3_fwd_x16_fused(src.p, B, S, S, l.cin, src.ld, _p(self.pk[key + "_x"]), amax_x,
                                     self._wamax(key), _p(self.pk[l.name + ".bpk_e"]), dst.p, dst.ld, l.cout, l.kc,
                                     self._slot(ws, l.dst_slot), {"resid": 1, "film": 2, "pool": 3}[l.kind],
                                     *resid, *film, self.nterm, s)

    def _gn_fwd(self, ws, P, name, y: Act, B, S, C, st, stats_from_conv, stream):
        lb = lib()
        nchunks = _cdiv(S * S, CHUNK)
        if not stats_from_conv:
            lb.cdm_reduce_stats(y.p, y.ld, B, S * S, C, CHUNK, _p(ws.slab), stream)
        cpg = C // GN_GROUPS
        lb.cdm_gn_fwd_finalize(_p(ws.slab), B, nchunks, 2, C, GN_GROUPS, float(S * S * cpg), _p(P[name + ".weight"]),
                               _p(P[name + ".bias"]), GN_EPS, _p(st["mean"]), _p(st["invstd"]), _p(st["scale"]),
                               _p(st["shift"]), stream)

    # ------------------------------------------------------------------------------------------
    # backward (train mode workspaces only)
    # ------------------------------------------------------------------------------------------
    def backward(self, ws: "Workspace", P, deps: torch.Tensor, G: Dict[str, torch.Tensor], stream: int,
                 out3_bias_done: bool = False, on_stage=None, dx: Optional[torch.Tensor] = None,
                 dt: Optional[torch.Tensor] = None, dc: Optional[torch.Tensor] = None,
                 stop_after: Optional[str] = None):
        """deps [B,H,W] = dL/d eps.  Writes (assigns) every parameter gradient into G[name].

        Optional input gradients (the module API under autograd, ContextUnet.py:42-60): dx [B,H,W] = dL/dx (the
        image), dt [rows_t] = dL/dt, dc [rows_c, n_cfeat] = dL/dc.  A t or c broadcast over the batch (one row) gets
        its embedding gradients summed over the samples.

        ``on_stage(name)`` is called (on the host, in stream order) as soon as the gradients of a stage
        are final: "out", "up2", "up1", "up0emb", "down2", "down1", "init" — used to start the
        data-parallel all-reduce of that stage while the rest of the backward runs.

        ``stop_after="up0emb"`` returns right after that stage's hook: dt and dc (and the gradients of out, up2, up1, up0
        and the embeddings) are final there, the down2 / down1 / init backward — which only feeds the encoder's
        parameter gradients and dx — is not launched, and those entries of G are left unwritten (the parameter fit,
        likelihood.ParamFit).  None runs everything."""
        assert stop_after in (None, "up0emb"), stop_after
        assert stop_after is None or dx is None, "dx is final only after the init stage"
        hook = on_stage or (lambda name: None)
        assert ws.train, "backward needs a train-mode workspace"
        lb = lib(); s = stream
        nf, H, B = self.nf, self.H, ws.B
        H2 = H // 4
        # ---------------- out.3 (nf -> 1) ----------------
        if self.cp > 1:
            gO = self._out3_bwd_c(ws, deps, G, s)
        else:
            R = cout1_band_rows(B, H)
            if self.fuses_gn_out():
                lb.cdm_conv3x3_cout1_wgrad_gn(_p(deps), _p(ws.yO), nf, B, H, H, nf, _p(ws.gnO["scale"]),
                                              _p(ws.gnO["shift"]), -R, _p(ws.slab), s)
            else:
                lb.cdm_conv3x3_cout1_wgrad(_p(deps), _p(ws.zO), nf, B, H, H, nf, -R, _p(ws.slab), s)
            S = fold(ws, _p(ws.slab), B * H // R, 9, nf, s)
            lb.cdm_slab_sum_all(_p(ws.dpart), S, 9, 0, 9, nf, _p(G["out.3.weight"]), 1, 9, 0, s)
            if not out3_bias_done:
                _sum_into(deps, G["out.3.bias"], ws, s)
            gO = ws.G0
            lb.cdm_conv3x3_cout1_dgrad(_p(deps), B, H, H, nf, _p(P["out.3.weight"]), _p(gO), nf, s)
        # ---------------- out.1 GroupNorm + ReLU ----------------
        dyO = ws.D0
        dslot = self._slot(ws, "dy:out.0")
        self._gn_bwd(ws, P, "out.1", "out.0.bias", Act(gO, nf), 0, Act(ws.yO, nf), B, H, nf, ws.gnO, None, 0,
                     Act(dyO, nf), G, s, amax=dslot)
        # ---------------- out.0 conv (2nf -> nf) ----------------
        self._wgrad3x3(ws, Act(dyO, nf), ws.catO, B, H, 2 * nf, nf, G["out.0.weight"], s, amax_dy=dslot,
                       amax_x=self._slot(ws, "catO"))
        self.conv3x3("out.0.wdg", _p(dyO), B, H, nf, nf, None, ws.dcatO.p, ws.dcatO.ld, 2 * nf, 0, None, 0,
                     self.kc_out0, s, amax_x=dslot, amax_y=self._slot(ws, ws.out0_g_key))
        hook("out")
        # ---------------- up2, up1 (its last conv carries FiLM2): the blocks, then the ConvT feeding them ----------
        for ct in reversed(self.convT):
            self._stage_bwd(ws, P, ct.stage, G, s)
            self._convT_bwd(ws, P, ct, G, s)
            hook(ct.stage)
        # ---------------- up0: GroupNorm + ReLU + FiLM1 ----------------
        c0 = 2 * nf
        rows_c, rows_t = ws.c_rows, ws.t_rows
        self._gn_bwd(ws, P, "up0.1", "up0.0.bias", ws.dcatU1.sl(0, c0), 2, Act(ws.y0, c0), B, H2, c0, ws.gn0,
                     ws.emb["contextembed1"], c0 if rows_c > 1 else 0, Act(ws.D2, c0), G, s,
                     film_out=(ws.d_emb["contextembed1"], ws.d_emb["timeembed1"]))
        # up0 weight: dW[ci][(ij,co)] = sum_n hv[n][ci] dy0[n][(ij,co)]  -> [ci][co][ij]
        KN = self.KK0 * c0
        if self.up0_large:
            # dy0 [B][ij][co] -> [B][co][ij]: the K order of W[ci][(co, ij)] (134 MB at config 5, not the weights)
            lb.cdm_transpose_batched(_p(ws.D2), B, self.KK0, c0, _p(ws.up0T), s)
            if B <= 16 and c0 % 64 == 0:
                lb.cdm_up0_wgrad(_p(ws.hv), B, c0, _p(ws.D2), self.KK0, _p(G["up0.0.weight"]), s)
                # input gradient over W in place (VALU, W read once): per-K-range partials folded over the splits
                sp = lb.raw("cdm_up0_dgrad_splits")(c0, self.KK0)
                lb.cdm_up0_dgrad(_p(ws.up0T), B, c0, _p(P["up0.0.weight"]), self.KK0, _p(ws.slab), s)
                lb.cdm_slab_reduce(_p(ws.slab), sp, B, c0, _p(ws.dhv), c0, 0, 1, c0, 0, 1.0, s)
                a_dy = None
            else:
                sp = lb.raw("cdm_gemm_splits")(B, 1)
                lb.cdm_gemm_tn_f32(_p(ws.hv), c0, c0, B, _p(ws.up0T), KN, KN, 1, _p(ws.slab), s)
                lb.cdm_slab_reduce(_p(ws.slab), sp, c0, KN, _p(G["up0.0.weight"]), KN, 0, 1, 0, 0, 1.0, s)
                wT = self.pk["up0.WT"] = self._buf("up0.WT", (KN, c0))
                lb.cdm_transpose(_p(P["up0.0.weight"]), c0, KN, _p(wT), s)
                a_dy, w_t = ws.up0T, wT
        else:
            sp = lb.raw("cdm_gemm_splits")(B, 1)
            lb.cdm_gemm_tn_f32(_p(ws.hv), c0, c0, B, _p(ws.D2), KN, KN, 1, _p(ws.slab), s)
            if sp == 1:   # [ci][ij][co] -> [ci][co][ij]: a batched tiled transpose
                lb.cdm_transpose_batched(_p(ws.slab), c0, self.KK0, c0, _p(G["up0.0.weight"]), s)
            else:
                lb.cdm_slab_reduce(_p(ws.slab), sp, c0, KN, _p(G["up0.0.weight"]), KN, 1, self.KK0, c0, 0, 1.0, s)
            a_dy, w_t = ws.D2, self.pk["up0.wtT"]
        # dhv[n][ci] = sum_k dy0[n][k] W[ci][k] over k = (ij, co) or (co, ij) (large)   (split-K over 16*16*2nf)
        if a_dy is not None:
            want = max(1, min(64, _cdiv(1024, _cdiv(B, 128) * _cdiv(c0, 128))))
            sp = lb.raw("cdm_gemm_splits")(KN, want)
            lb.cdm_gemm_f32(_p(a_dy), KN, B, KN, _p(w_t), c0, c0, _p(ws.dhv), c0, None, 1, 0, sp,
                            _p(ws.slab), s)
            if sp > 1:
                lb.cdm_slab_reduce(_p(ws.slab), sp, B, c0, _p(ws.dhv), c0, 0, 1, c0, 0, 1.0, s)
        # to_vec: d2 grad += dhv * gelu'(hpre) / (h/4)^2
        d2g = ws.dcatU1.sl(2 * nf, 2 * nf)
        lb.cdm_avgpool_gelu_bwd(_p(ws.dhv), _p(ws.hpre), B, H2 * H2, c0, d2g.p, d2g.ld, s)
        # ---------------- embeddings ----------------
        d = ws._mlp
        for k, m in enumerate(MLPS):
            md = d.m[k]
            dout = ws.d_emb[m]
            if md.rows == 1 and B > 1:          # t / c broadcast over the batch: one embedding row, sums over samples
                E = dout.shape[1]
                lb.cdm_col_sum(_p(dout), B, E, _p(ws.d_emb_row[m]), 0, s)
                dout = ws.d_emb_row[m]
            md.dout = _p(dout); md.dpre = _p(ws.emb_dpre[m])
            md.dw1 = _p(G[m + ".model.0.weight"]); md.db1 = _p(G[m + ".model.0.bias"])
            md.dw2 = _p(G[m + ".model.2.weight"]); md.db2 = _p(G[m + ".model.2.bias"])
        lb.cdm_embed_bwd(ctypes_addr(d), s)
        for dv, (ma, mb), rows, in_dim in ((dt, ("timeembed1", "timeembed2"), ws.t_rows, 1),
                                           (dc, ("contextembed1", "contextembed2"), ws.c_rows, self.ncf)):
            if dv is not None:
                lb.cdm_embed_input_grad(_p(ws.emb_dpre[ma]), _p(P[ma + ".model.0.weight"]), 2 * nf,
                                        _p(ws.emb_dpre[mb]), _p(P[mb + ".model.0.weight"]), nf, rows, in_dim, _p(dv), s)
        hook("up0emb")
        if stop_after == "up0emb":
            return
        # ---------------- down2, down1, init ----------------
        for stage in ("down2", "down1"):
            self._stage_bwd(ws, P, stage, G, s)
            hook(stage)
        self._stage_bwd(ws, P, "init", G, s)
        if dx is not None:
            if self.cp > 1:
                self._image_grad_c(ws, dx, s)
            else:
                self._image_grad(ws, P, dx, s)
        hook("init")

    def _out3_bwd_c(self, ws, deps: torch.Tensor, G, s: int):
        """out.3 = Conv2d(n_feat, in_channels > 1) backward on the general kernels; deps = dL/d eps, NHWC [B*H*W, cp] with
        zero padding channels.  Returns the gradient wrt zO = relu(GN(yO)) (ws.G0)."""
        lb = lib()
        nf, H, B, cp, C = self.nf, self.H, ws.B, self.cp, self.cimg
        zslot = self._slot(ws, "zO")
        gw = self._buf("out.3.gwpad", (cp, nf, 3, 3))
        self._wgrad3x3(ws, Act(deps, cp), Act(ws.zO, nf), B, H, nf, cp, gw, s, amax_x=zslot)
        G["out.3.weight"].copy_(gw[:C])
        gb = self._buf("out.3.gbpad", (cp,))
        lb.cdm_reduce_sum(_p(deps), cp, B, H * H, cp, CHUNK, _p(ws.slab), s)
        nparts = fold(ws, _p(ws.slab), B * _cdiv(H * H, CHUNK), 1, cp, s)
        lb.cdm_slab_sum_all(_p(ws.dpart), nparts, 1, 0, 1, cp, _p(gb), 0, 1, 0, s)
        G["out.3.bias"].copy_(gb[:C])
        gO = ws.G0
        self.conv3x3("out.3.wdg", _p(deps), B, H, cp, cp, None, _p(gO), nf, nf, 0, None, 0, conv_kc(cp, nf), s)
        return gO

    def _image_grad_c(self, ws, dx: torch.Tensor, s: int):
        """dL/dx for in_channels > 1 (NHWC [B*H*W, cp]): init_conv.conv1's input gradient (its dgrad, already in
        its plan's dgrad_dst) plus the random 1x1 shortcut's, dx[p][k] += sum_n g_res[p][n] w[n][k] (one GEMM)."""
        lb = lib()
        nf, H, B, cp, C = self.nf, self.H, ws.B, self.cp, self.cimg
        P0 = B * H * H
        gd = ws.plan[0].dgrad_dst
        dx.view(P0, cp).copy_(gd.buf.view(-1)[: P0 * gd.ld].view(P0, gd.ld)[:, :cp])
        sc_w, _, split = ws.sc_pending
        assert split >= B, "input gradients with two shortcut draws (CFG halves) are not a module-call form"
        wpad = self._buf("sc.wpad", (nf, cp))
        wpad[:, C:].zero_(); wpad[:, :C].copy_(sc_w[: nf * C].view(nf, C))
        gres = ws.plan[1].gout
        sp = lib().raw("cdm_gemm_splits")(nf, 1)
        lb.cdm_gemm_f32(gres.p, gres.ld, P0, nf, _p(wpad), cp, cp, _p(dx), cp, None, 1, EPI_ACCUM, sp, _p(ws.slab), s)

    def _image_grad(self, ws, P, dx: torch.Tensor, s: int):
        """dL/dx of the image (ResidualConvBlock(1, nf, is_res) at diffusion_utilities.py:45-55 under autograd):
        init_conv.conv1's input gradient (the tap-flipped 3x3 conv over its BatchNorm + ReLU backward, applied while
        reading g and y) plus the random 1x1 shortcut's (sum_c w[c] * grad of the block output).  Runs after the init
        conv's backward, whose BatchNorm coefficients ws.coef still hold."""
        p, l = ws.plan[0], self.layers[0]
        C, B, H = l.cout, ws.B, self.H
        st, co = p.bn, ws.coef
        g, gres = p.gout, ws.plan[1].gout
        sc_w, _, split = ws.sc_pending
        lib().cdm_conv3x3_cin1_dgrad(g.p, g.ld, _p(p.y), C, _p(st["scale"]), _p(st["shift"]), _p(st["mean"]),
                                     _p(st["invstd"]), _p(co[0]), _p(co[1]), _p(co[2]), _p(P[l.w]), gres.p, gres.ld,
                                     _p(sc_w), split, B, H, H, C, _p(dx), s)

    def _stage_bwd(self, ws, P, stage, G, s):
        for l in reversed(self.stages[stage]):
            self._conv_bn_bwd(ws, ws.plan[l.index], P, G, s)

    def _conv_bn_bwd(self, ws, p: "LayerPlan", P, G, s):
        lb = lib()
        l, g, y, st = p.l, p.gout, p.y, p.bn
        B, S, C = ws.B, l.S, l.cout
        mode = {"pool": 1, "film": 2}.get(l.kind, 0)
        film_a, film_an = None, 0
        if mode == 2:
            film_a, film_an = ws.emb["contextembed2"], (C if ws.c_rows > 1 else 0)
        HWp = (S // 2) * (S // 2) if mode == 1 else S * S
        nch = _cdiv(HWp, CHUNK)
        co = ws.coef
        bn = l.bn
        if p.sums_by:
            # the sums came with the consumer's weight gradient (PreBnReluSums): one partial per block
            assert mode == 0
            nparts = fold(ws, _p(ws.sums), p.sums_parts, 5, C, s)
        else:
            assert not p.own16, "bf16 activations need the fused BN-backward sums"
            lb.cdm_norm_bwd_reduce(mode, g.p, g.ld, _p(y), C, B, S, S, C, _p(st["scale"]), _p(st["shift"]), 0,
                                   _p(st["mean"]), _p(st["invstd"]), 0, 1, _p(film_a), film_an, CHUNK, _p(ws.slab), s)
            if mode == 2:  # FiLM2 sums -> d cemb2 / d temb2 (per sample)
                lb.cdm_slab_sum_nc(_p(ws.slab), B, nch, 5, 2, C, _p(ws.d_emb["contextembed2"]), s)
                lb.cdm_slab_sum_nc(_p(ws.slab), B, nch, 5, 3, C, _p(ws.d_emb["timeembed2"]), s)
            nparts = fold(ws, _p(ws.slab), B * nch, 5, C, s)
        fin = lb.cdm_bn_bwd_finalize_frozen if ws.frozen else lb.cdm_bn_bwd_finalize
        fin(_p(ws.dpart), nparts, C, float(B * S * S), _p(P[bn + ".weight"]), _p(st["invstd"]), _p(G[bn + ".weight"]),
            _p(G[bn + ".bias"]), _p(co[0]), _p(co[1]), _p(co[2]), _p(G[l.b]), s)
        coef = (_p(st["scale"]), _p(st["shift"]), _p(st["mean"]), _p(st["invstd"]), _p(co[0]), _p(co[1]), _p(co[2]))
        if l.cin == 1:
            # init_conv.conv1: only a weight gradient (the input needs none); its BN backward runs while that kernel
            # reads g and y (dy is never written)
            lb.cdm_conv3x3_cin1_wgrad_bnbwd(g.p, g.ld, _p(y), C, *coef, _p(ws.x_in), B, S, S, C, CHUNK, _p(ws.slab), s)
            nparts = fold(ws, _p(ws.slab), B * _cdiv(S * S, CHUNK), 10, C, s)
            lb.cdm_slab_sum_all(_p(ws.dpart), nparts, 10, 0, 9, C, _p(G[l.w]), 1, 9, 0, s)
            return
        # the dgrad goes first: it writes the producer's g, which the weight gradient's producer sums read
        gslot = self._slot(ws, p.g_slot)
        dslot = self._slot(ws, "dy:" + l.name)
        dgd, key = p.dgrad_dst, l.name + ".wdg"
        accum = EPI_ACCUM if p.dgrad_accum else 0
        if p.fused:
            # dy = bn_bwd(g, y) goes from the dgrad to the weight gradient through ws.dyo (g's row stride and element
            # type), never through a per-layer buffer; its h3 scale comes from a bound on max|dy|
            if self.h3:
                lb.cdm_bn_bwd_amax_bound(C, _p(co[0]), _p(co[1]), _p(co[2]), _p(st["mean"]), _p(st["invstd"]),
                                         self._slot(ws, "g:" + l.name), self._slot(ws, "y:" + l.name), dslot, s)
            if self.nterm == 1:
                # one-term (bf16) arithmetic: dy by its own elementwise pass, then the dgrad on the LDS-halo forward
                # schedule (halo two chunks ahead, one barrier per chunk)
                lb.cdm_bn_bwd_dy(g.p, g.ld, _p(y), C, B * S * S, C, *coef, _p(ws.dyo), g.ld, p.own16 | (p.own16 << 1), s)
                self.conv3x3(key, _p(ws.dyo), B, S, C, g.ld, None, dgd.p, dgd.ld, l.cin, accum, None, 0, l.kc, s,
                             amax_y=gslot, dt=p.dt_dgrad)
            else:
                lb.cdm_conv3x3_dgrad_x16_bnbwd_dy(g.p, g.ld, _p(y), C, *coef, B, S, S, C, _p(self.pk[key + "_x"]),
                                                  dslot, self._wamax(key), dgd.p, dgd.ld, l.cin, accum, gslot,
                                                  _p(ws.dyo), self.nterm, p.dt_dgrad, s)
            self._wgrad_rows(ws, p, _p(ws.dyo), g.ld, dslot, G[l.w], s)
            return
        dy = p.dy
        lb.cdm_norm_apply_bwd(mode, g.p, g.ld, _p(y), C, B, S, S, C, _p(st["scale"]), _p(st["shift"]), 0,
                              _p(st["mean"]), _p(st["invstd"]), 0, 1, _p(film_a), film_an, _p(co[0]), _p(co[1]),
                              _p(co[2]), 0, dy.p, dy.ld, dslot, s)
        self.conv3x3(key, dy.p, B, S, C, dy.ld, None, dgd.p, dgd.ld, l.cin, accum, None, 0, l.kc, s, amax_x=dslot,
                     amax_y=gslot, dt=p.dt_dgrad)
        pad0 = l.index == 0 and self.cp > self.cimg             # the init conv's zero image-channel columns
        gW = self._buf("init.gwpad", (C, self.cp, 3, 3)) if pad0 else G[l.w]
        if p.pre is not None:
            self._wgrad_rows(ws, p, dy.p, dy.ld, dslot, gW, s)
        else:
            self._wgrad3x3(ws, dy, p.src, B, S, l.cin, C, gW, s, amax_dy=dslot, amax_x=self._slot(ws, l.src_slot))
        if pad0:
            G[l.w].copy_(gW[:, :self.cimg])

    def _wgrad_rows(self, ws, p: "LayerPlan", dy_p, lddy, amax_dy, gW, s):
        """Kernel-row weight gradient of p's layer into gW (OIHW) from a stored dy [pix][C_out] (row stride lddy).  X is
        the plan's source: plain, or relu(x s + t) of a fused producer's y (p.pre), whose BN-backward channel sums then
        ride along where the plan says so (p.sums_from: the producer's g was written by this layer's dgrad)."""
        lb = lib()
        l, x, q = p.l, p.src, p.sums_from
        B, S, C = ws.B, l.S, l.cout
        x_s, x_t = p.pre or (None, None)
        sums = (q.gout.p, q.gout.ld, _p(q.bn["mean"]), _p(q.bn["invstd"]), _p(ws.sums)) if q else (None, 0) + (None,) * 3
        lb.cdm_conv3x3_wgrad_x16_ex(dy_p, lddy, None, 0, *(None,) * 7, C, x.p, B, S, S, l.cin, x.ld, x_s, x_t, *sums,
                                    amax_dy, self._slot(ws, l.src_slot), p.sp, _p(ws.slab), self.nterm, p.dt_wgrad, s)
        # slab[z][co][tap*cin+ci] -> OIHW [co][ci][tap]
        lb.cdm_slab_reduce(_p(ws.slab), p.sp, C, 9 * l.cin, _p(gW), 9 * l.cin, 1, 9, l.cin, 0, 1.0, s)

    def _wgrad3x3(self, ws, dy: Act, x: Act, B, S, cin, cout, gW, s, amax_dy=None, amax_x=None):
        """Weight gradient of a 3x3 conv on the split-K GEMMs of this engine's arithmetic, folded into gW (OIHW)."""
        lb = lib()
        sp = wgrad_splits(B * S * S, cout, 9 * cin)
        if S % 8:
            # the 16-bit weight-gradient GEMMs stage 8-pixel pieces of one image row: other widths take the fp32 GEMM
            lb.cdm_conv3x3_wgrad(dy.p, dy.ld, cout, x.p, B, S, S, cin, x.ld, sp, _p(ws.slab), s)
        elif self.x16:
            am = _p(self._amax)
            if self.h3 and amax_dy is None:
                amax_dy = am
                lb.cdm_amax_f32(dy.p, B * S * S, cout, dy.ld, amax_dy, 0, s)
            if self.h3 and amax_x is None:
                amax_x = am + 4
                lb.cdm_amax_f32(x.p, B * S * S, cin, x.ld, amax_x, 0, s)
            lb.cdm_conv3x3_wgrad_x16(dy.p, dy.ld, cout, x.p, B, S, S, cin, x.ld, amax_dy, amax_x, sp, _p(ws.slab),
                                     self.nterm, s)
        elif self.nterm:
            lb.cdm_conv3x3_wgrad_x3(dy.p, dy.ld, cout, x.p, B, S, S, cin, x.ld, sp, _p(ws.slab), self.nterm, s)
        else:
            lb.cdm_conv3x3_wgrad(dy.p, dy.ld, cout, x.p, B, S, S, cin, x.ld, sp, _p(ws.slab), s)
        # slab[z][co][tap*cin+ci] -> OIHW [co][ci][tap]
        lb.cdm_slab_reduce(_p(ws.slab), sp, cout, 9 * cin, _p(gW), 9 * cin, 1, 9, cin, 0, 1.0, s)

    def _convT_bwd(self, ws, P, ct: ConvTSpec, G, s):
        """ConvTranspose2d(cin, nf, 2, 2) backward; the grad of its output [B, 2Hin, 2Hin, nf] is where its consumer's
        dgrad wrote it."""
        lb = lib()
        name, B, Hin, cin, cout = ct.name, ws.B, ct.Hin, ct.cin, self.nf
        gy, x, dx = ws.plan[ct.consumer.index].dgrad_dst, getattr(ws, ct.src), getattr(ws, "d" + ct.src)
        Ho = 2 * Hin
        lb.cdm_reduce_sum(gy.p, gy.ld, B, Ho * Ho, cout, CHUNK, _p(ws.slab), s)
        nparts = fold(ws, _p(ws.slab), B * _cdiv(Ho * Ho, CHUNK), 1, cout, s)
        lb.cdm_slab_sum_all(_p(ws.dpart), nparts, 1, 0, 1, cout, _p(G[name + ".bias"]), 0, 1, 0, s)
        sp = wgrad_splits(B * Hin * Hin, cin, 4 * cout)
        if self.x16 and Hin % 8 == 0:
            a_gy = self._slot(ws, ct.g_slot)
            lb.cdm_convT2x2_wgrad_x16(x.p, B, Hin, Hin, cin, x.ld, gy.p, cout, gy.ld, self._slot(ws, ct.src), a_gy, sp,
                                      _p(ws.slab), self.nterm, s)
        else:   # fp32 arithmetic, or an input grid whose width is not a multiple of 8 (the 16-bit GEMM's pieces)
            lb.cdm_convT2x2_wgrad(x.p, B, Hin, Hin, cin, x.ld, gy.p, cout, gy.ld, sp, _p(ws.slab), s)
        # slab[z][ci][ij*cout+co] -> [ci][co][ij]
        lb.cdm_slab_reduce(_p(ws.slab), sp, cin, 4 * cout, _p(G[name + ".weight"]), 4 * cout, 1, 4, cout, 0, 1.0, s)
        if self.x16:
            lb.cdm_convT2x2_dgrad_x16(gy.p, B, Hin, Hin, cout, gy.ld, _p(self.pk[name + ".wtT_x"]),
                                      self._slot(ws, ct.g_slot), self._wamax(name + ".wtT"), dx.p, dx.ld, cin, 0,
                                      self.nterm, s)
        else:
            lb.cdm_convT2x2_dgrad(gy.p, B, Hin, Hin, cout, gy.ld, _p(self.pk[name + ".wtT"]), dx.p, dx.ld, cin, 0, s)

    def _gn_bwd(self, ws, P, name, bias_name, g: Act, mode, y: Act, B, S, C, st, film_a, film_an, dy: Act, G, s,
                film_out=None, amax=None):
        lb = lib()
        nch = _cdiv(S * S, CHUNK)
        cpg = C // GN_GROUPS
        lb.cdm_norm_bwd_reduce(mode, g.p, g.ld, y.p, y.ld, B, S, S, C, _p(st["scale"]), _p(st["shift"]), C,
                               _p(st["mean"]), _p(st["invstd"]), GN_GROUPS, cpg, _p(film_a), film_an, CHUNK,
                               _p(ws.slab), s)
        if film_out is not None:
            lb.cdm_slab_sum_nc(_p(ws.slab), B, nch, 5, 2, C, _p(film_out[0]), s)
            lb.cdm_slab_sum_nc(_p(ws.slab), B, nch, 5, 3, C, _p(film_out[1]), s)
        co = ws.gcoef
        lb.cdm_gn_bwd_finalize(_p(ws.slab), B, nch, C, GN_GROUPS, float(S * S * cpg), S * S, _p(P[name + ".weight"]),
                               _p(st["invstd"]), _p(co[0]), _p(co[1]), _p(co[2]), _p(co[3]), _p(co[4]), _p(co[5]), s)
        lb.cdm_col_sum3(_p(co[3]), _p(G[name + ".weight"]), _p(co[4]), _p(G[name + ".bias"]),
                        _p(co[5]) if bias_name is not None else None,
                        _p(G[bias_name]) if bias_name is not None else None, B, C, s)
        lb.cdm_norm_apply_bwd(mode, g.p, g.ld, y.p, y.ld, B, S, S, C, _p(st["scale"]), _p(st["shift"]), C,
                              _p(st["mean"]), _p(st["invstd"]), GN_GROUPS, cpg, _p(film_a), film_an, _p(co[0]),
                              _p(co[1]), _p(co[2]), C, dy.p, dy.ld, amax, s)


def _sum_into(x: torch.Tensor, out: torch.Tensor, ws, stream: int):
    """out[0] = sum(x) for a C=1 map: C=4 column partials over a [n/4, 4] view, then fold."""
    lb = lib()
    n = x.numel()
    assert n % 4 == 0
    nch = _cdiv(n // 4, CHUNK)
    scratch = ws.slab
    lb.cdm_reduce_sum(_p(x), 4, 1, n // 4, 4, CHUNK, _p(scratch), stream)
    part = scratch[4 * nch: 4 * nch + 4]
    S = fold(ws, _p(scratch), nch, 1, 4, stream)
    lb.cdm_slab_sum_all(_p(ws.dpart), S, 1, 0, 1, 4, _p(part), 0, 1, 0, stream)
    lb.cdm_col_sum(_p(part), 4, 1, _p(out), 0, stream)


def fold(ws, slab_ptr: int, ntiles: int, R: int, C: int, stream: int) -> int:
    """Stage-1 parallel fold of an fp32 partial slab [ntiles][R][C] into fp64 parts; returns #parts."""
    S = max(1, min(ntiles, max(1, 512 // _cdiv(C, 64)), ws.dpart.numel() // max(1, R * C)))
    lib().cdm_slab_colsum(slab_ptr, ntiles, R, C, _p(ws.dpart), S, stream)
    return S


def cout1_band_rows(B: int, H: int) -> int:
    """Rows per block of the out.3 weight-gradient band kernel: the largest divisor of H that still gives >= 1024
    blocks (B=256 at 64x64: 16 rows -> 1024 blocks)."""
    R = H
    while R > 1 and (B * H // R < 1024 or H % R):
        R -= 1
    return R


def wgrad_splits(K: int, M: int, N: int) -> int:
    """Split-K factor for a weight-gradient GEMM (M = C_out, N = 9 C_in for a 3x3 conv, K = pixels).

    3x3 convs with C_in, C_out % 128 == 0 run the kernel-row weight gradient: 3 (C_out/128) (C_in/128) blocks per split,
    one 512-thread block per CU at a time, all blocks equal work — so the grid is sized to whole rounds of 256 CUs
    (768 blocks): 228 splits gave 684 blocks = 2.67 rounds, whose last round ran a third empty (same-box A/B,
    profiles/r3_ab_wgrad_rounds.txt: C2 train step 53.04 -> 51.89 ms, C4 33.09 -> 32.12 ms).  Others: ~2048
    workgroups of the generic split GEMM."""
    if N % 9 == 0 and M % 128 == 0 and (N // 9) % 128 == 0:
        per = 3 * (M // 128) * ((N // 9) // 128)
        want = max(1, min(512, round(WGRAD_BLOCKS / per)))
        return lib().raw("cdm_gemm_splits")(K, want)
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    want = max(1, min(512, _cdiv(2048, tiles)))
    return lib().raw("cdm_gemm_splits")(K, want)


def ctypes_addr(obj):
    import ctypes
    return ctypes.addressof(obj)


class LayerPlan:
    """What the launches of one conv layer need in one workspace, resolved once (Workspace.__init__).

    y, bn: the pre-norm output and the BatchNorm coefficient tensors.  src / dst: input and output activations; pre =
    (scale, shift) pointers where a fused producer hands over its y for src (the staging applies BN + ReLU).
    fused_fwd: this layer's own apply runs in its consumer's staging; ymm: (pointer, ld) of its max / min keys (h3).
    Train: gout = the gradient of its output, dy its BN-backward buffer (non-fused), dgrad_dst / dgrad_accum where its
    input gradient goes, g_slot the amax-slot key that dgrad output records into; fused: BN backward inside the dgrad;
    sums_from: the producer's plan whose BN-backward sums this layer's weight gradient accumulates (that plan:
    sums_by, sums_parts partials); sp: split-K factor of its weight gradient; own16: y and g stored as bf16;
    dt_fwd / dt_dgrad / dt_wgrad: the dtype bits of its three conv launches."""
    __slots__ = ("l", "y", "bn", "src", "pre", "dst", "fused_fwd", "ymm", "gout", "dy", "dgrad_dst", "dgrad_accum",
                 "g_slot", "fused", "sums_from", "sums_by", "sums_parts", "sp", "own16", "dt_fwd", "dt_dgrad",
                 "dt_wgrad")

    def __init__(self, l: LayerSpec):
        self.l = l
        self.y = self.bn = self.src = self.pre = self.dst = self.ymm = self.gout = self.dy = self.dgrad_dst = None
        self.g_slot = self.sums_from = None
        self.fused_fwd = self.dgrad_accum = self.fused = self.sums_by = False
        self.sums_parts = self.sp = self.own16 = self.dt_fwd = self.dt_dgrad = self.dt_wgrad = 0


class Workspace:
    """All device buffers for one batch size and mode (train keeps what backward needs)."""

    def __init__(self, eng: UNetEngine, B: int, train: bool, frozen: bool = False):
        self.eng, self.B, self.train = eng, B, train
        self.frozen = False          # set by each forward (eval-mode BatchNorm in a train-structured forward)
        dev = eng.device
        nf, H, ncf = eng.nf, eng.H, eng.ncf
        H1, H2 = H // 2, H // 4
        P0, P1, P2 = B * H * H, B * H1 * H1, B * H2 * H2
        E = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        self.catO = Act(E(P0, 2 * nf), 2 * nf)
        self.catU2 = Act(E(P1, 2 * nf), 2 * nf)
        self.catU1 = Act(E(P2, 4 * nf), 4 * nf)
        self.eps = E(B, H, H) if eng.cp == 1 else E(P0, eng.cp)
        self.yT1 = E(P1, nf)
        self.yT2 = E(P0, nf)
        self.y0 = E(P2, 2 * nf)
        self.yO = E(P0, nf)
        # zO = relu(GN(yO)) only exists where out.3 cannot apply out.1 in its staging (537 MB at the bench shape)
        self.zO = E(P0, nf) if not eng.fuses_gn_out() else torch.empty(0, device=dev)
        self.hsum, self.hpre, self.hv = E(B, 2 * nf), E(B, 2 * nf), E(B, 2 * nf)
        self.c_zero = torch.zeros(B, ncf, device=dev)
        self.emb = {m: E(B, (2 if m.endswith("1") else 1) * nf) for m in MLPS}
        if train:
            self.emb_pre = {m: E(B, (2 if m.endswith("1") else 1) * nf) for m in MLPS}
            self.emb_h = {m: E(B, (2 if m.endswith("1") else 1) * nf) for m in MLPS}
            self.emb_dpre = {m: E(B, (2 if m.endswith("1") else 1) * nf) for m in MLPS}
            self.d_emb = {m: E(B, (2 if m.endswith("1") else 1) * nf) for m in MLPS}
            self.d_emb_row = {m: E(1, (2 if m.endswith("1") else 1) * nf) for m in MLPS}   # broadcast t / c
        self.gn0 = {k: E(B * 2 * nf) for k in ("mean", "invstd", "scale", "shift")}
        self.gnO = {k: E(B * nf) for k in ("mean", "invstd", "scale", "shift")}
        # per conv-BN layer: its plan — y (pre-norm), BN coefficients, source and destination
        L = eng.layers
        self.plan = [LayerPlan(l) for l in L]
        self._no_z = torch.empty(0, device=dev)
        for p in self.plan:
            p.y = E(B * p.l.S * p.l.S, p.l.cout)
            p.bn = {k: E(p.l.cout) for k in ("mean", "invstd", "scale", "shift")}
        self.y = {p.l.name: p.y for p in self.plan}
        self.bn = {p.l.name: p.bn for p in self.plan}
        self.dst_kind = {l.name: l.kind for l in L}
        self.fused_fwd = {l.name for l in L if train and eng.fuses_bn_fwd(l, l.kind, B)}
        for p in self.plan:
            l = p.l
            p.fused_fwd = l.name in self.fused_fwd
            if l.dst is not None:
                p.dst = self._view(l.dst)
            else:      # a fused producer's z is never materialised (the consumer stages relu(y s + t) itself)
                p.dst = Act(self._no_z if p.fused_fwd else E(B * l.S * l.S, l.cout), l.cout)
            if l.src is not None:
                p.src = self._view(l.src)
            elif l.prev is not None:                 # (layer 0 reads the image: cdm_conv3x3_cin1_*, or set per forward)
                q = self.plan[l.prev.index]
                p.src = q.dst
                if q.fused_fwd:                      # the producer hands over its pre-norm output and (scale, shift)
                    p.src, p.pre = Act(q.y, l.cin), (_p(q.bn["scale"]), _p(q.bn["shift"]))
        self.dst = {p.l.name: p.dst for p in self.plan}     # by name, like y and bn (tools, tests)
        self.slab = E(self._slab_floats())
        # per fused layer: max / min keys of its pre-norm output ([2][n_fused][Cmax] int32, refilled every forward):
        # p.ymm = (pointer, ld) of the layer's max keys; its min keys sit ld ints further
        Cmax = max(l.cout for l in L)
        self.ymm = torch.empty(2 * max(1, len(self.fused_fwd)) * Cmax, dtype=torch.int32, device=dev)
        if eng.h3:
            for i, p in enumerate(sorted((p for p in self.plan if p.fused_fwd), key=lambda p: p.l.name)):
                p.ymm = (self.ymm.data_ptr() + 4 * i * Cmax, self.ymm.numel() // 2)
        self.amax = torch.zeros(192, device=dev)  # h3 operand maxima, one slot per producer (UNetEngine._slot)
        self.aslot = {}
        self.dpart = torch.empty(10 * 32768 + 4096, device=dev, dtype=torch.float64)
        self.sc_pending = None
        self.fused, self.out0_g_key, self.sums_from, self.act16, self.dyo = set(), None, {}, set(), None
        if not train:
            return
        C4 = 4 * nf
        self.G0, self.D0 = E(P0, 2 * nf), E(P0, 2 * nf)
        self.G1, self.D1 = E(P1, 2 * nf), E(P1, 2 * nf)
        self.D2 = E(P2, 4 * nf)
        self.dcatO = Act(E(P0, 2 * nf), 2 * nf)
        self.dcatU2 = Act(E(P1, 2 * nf), 2 * nf)
        self.dcatU1 = Act(E(P2, 4 * nf), 4 * nf)
        self.dhv = E(B, 2 * nf)
        self.up0T = E(P2, 2 * nf) if eng.up0_large else None   # dy0 with (co, ij) order (large up0)
        self.coef = [E(C4) for _ in range(3)]
        self.gcoef = [E(B * C4) for _ in range(6)]
        # backward wiring: the grad of each layer's output (gout: the dcat* slice of a cat* destination, else written
        # by the next layer's dgrad), its dy buffer and where its own dgrad goes (accumulating into the dcat* slice of a
        # cat* source: the skip connection's other gradient is already there)
        pairs = {H: (self.G0, self.D0), H1: (self.G1, self.D1)}
        for p in self.plan:
            l = p.l
            Gb, Db = pairs[l.S]
            p.dy = Act(Db, l.cout)
            p.gout = self._view(l.dst, grad=True) if l.dst is not None else Act(Gb, l.cout)
            if l.src is not None and l.src[0].startswith("cat"):
                p.dgrad_dst, p.dgrad_accum = self._view(l.src, grad=True), True
            elif l.cin > 1:
                p.dgrad_dst = Act(Gb, l.cin)
            if l.cin > 1:
                p.sp = wgrad_splits(B * l.S * l.S, l.cout, 9 * l.cin)
        for ct in eng.convT:       # the grad wrt a ConvT output also records its max, for the h3 ConvT backward
            self.plan[ct.consumer.index].g_slot = ct.g_slot
        self._wire_fused_bn_bwd(pairs)
        # the fused layers' dy: one buffer, rewritten by each fused layer's dgrad and read by its weight gradient
        # right after; g's row stride (fp32 size, bf16 dy use half)
        if self.fused:
            self.dyo = E(max(B * p.l.S * p.l.S * p.gout.ld for p in self.plan if p.fused))
        # producer BN-backward sums in the consumer's weight gradient: a fused (BN-ReLU staged) dense producer q
        # whose consumer p takes the kernel-row weight gradient with the X transform; one partial per block of that
        # weight gradient: split x kernel row x co tile
        if eng.fuse_bn_sums:
            for p in self.plan[1:]:
                q, c = self.plan[p.l.index - 1], p.l
                if q.fused_fwd and c.cin % 128 == 0 and c.cout % 128 == 0 and c.S % 16 == 0:
                    p.sums_from, q.sums_by, q.sums_parts = q, True, p.sp * 3 * (c.cout // 128)
                    self.sums_from[c.name] = q.l.name
        self.sums = E(max([p.sums_from.sums_parts * 5 * p.l.cin for p in self.plan if p.sums_from] + [1]))
        # bf16 activations (C4): the fused chain's y and g (layers whose BN-ReLU apply runs in the next conv's
        # staging, C_in > 1; each has its BN-backward sums fused into the consumer's weight gradient and a private
        # gradient buffer, so every kernel reading them is one of the two templated conv kernels)
        if eng.act16 and not frozen:
            self.act16 = {p.l.name for p in self.plan if p.fused_fwd and p.l.cin > 1 and p.sums_by and p.fused
                          and p.gout.off == 0}
        # dtype bits of the launches (include/cdm_hip.h, "dt"): a layer in act16 stores y and g as bf16; its consumer
        # stages that y (forward, weight-gradient X) and writes that g (dgrad output, unless it accumulates elsewhere)
        for p in self.plan:
            q = self.plan[p.l.index - 1] if p.l.index else None
            p.own16 = int(p.l.name in self.act16)
            prod16 = q.own16 if q is not None else 0
            out16 = prod16 if (prod16 and not p.dgrad_accum and p.dgrad_dst.buf is q.gout.buf) else 0
            p.dt_fwd = prod16 | (p.own16 << 1)
            p.dt_dgrad = p.own16 | (out16 << 1)
            p.dt_wgrad = p.own16 | (prod16 << 1)

    def _view(self, sym, grad: bool = False) -> Act:
        """The activation view a LayerSpec names as (buffer, first channel, channels) in units of n_feat; grad: the same
        slice of the buffer's gradient."""
        name, c0, C = sym
        nf, b = self.eng.nf, getattr(self, "d" + name if grad else name)
        return b.sl(c0 * nf, C * nf) if isinstance(b, Act) else Act(b, C * nf)

    def _wire_fused_bn_bwd(self, pairs):
        """Fused layers read g and write their dgrad without a dy buffer in between, so g and the dgrad output
        must differ: walking the backward order, each fused layer writes its dgrad into the other buffer of its
        resolution's pair (G, D), which becomes the g of the layer before it (or of the ConvT that feeds it).  Non-fused
        layers keep dy in D (in place when their g already sits in D: the mode-0 apply is elementwise, index for
        index).  The dgrad that writes a fused layer's g (the next layer's; out.0's for the last) records max|g| for
        the layer's dy bound."""
        eng = self.eng
        self.fused = {l.name for l in eng.layers if eng.fuses_bn_bwd(l, l.kind, self.B)}
        for p in reversed(self.plan):
            l = p.l
            p.fused = l.name in self.fused
            if not p.fused:
                continue
            if l.next is not None:
                nxt = self.plan[l.next.index]
                assert nxt.g_slot is None
                nxt.g_slot = "g:" + l.name
            else:
                self.out0_g_key = "g:" + l.name
            if p.dgrad_accum:
                continue                                  # the dgrad accumulates into a concat-grad slice
            # g of a "plain" / "resid" layer is a slice of the concat gradient: any buffer of the pair is free
            G_, D_ = pairs[l.S]
            dst = D_ if p.gout.buf is G_ else G_
            p.dgrad_dst = Act(dst, l.cin)
            if l.src is None:
                assert l.prev.kind == "dense", l.prev.name
                self.plan[l.prev.index].gout = Act(dst, l.cin)


    def _slab_floats(self):
        eng, B = self.eng, self.B
        nf, H = eng.nf, eng.H
        P0 = B * H * H
        need = _cdiv(P0, CHUNK) * 10 * 2 * nf          # stats / bwd partials at full res (R <= 10)
        need = max(need, B * H // cout1_band_rows(B, H) * 9 * nf)   # out.3 weight-gradient band partials
        if self.train:
            for l in eng.layers:                         # conv wgrad split-K slabs
                if l.cin > 1:
                    sp = wgrad_splits(B * l.S * l.S, l.cout, 9 * l.cin)
                    need = max(need, sp * l.cout * 9 * l.cin)
            # out.0 (2nf -> nf at full resolution; not in eng.layers)
            need = max(need, wgrad_splits(P0, nf, 9 * 2 * nf) * nf * 9 * 2 * nf)
            if eng.cp > 1:                                  # out.3 (nf -> in_channels) on the general weight gradient
                need = max(need, wgrad_splits(P0, eng.cp, 9 * nf) * eng.cp * 9 * nf)
            for cin, Hin in ((4 * nf, H // 4), (2 * nf, H // 2)):   # convT wgrad
                need = max(need, wgrad_splits(B * Hin * Hin, cin, 4 * nf) * cin * 4 * nf)
            if not (eng.up0_large and B <= 16):             # up0 weight grad through a split-K slab
                need = max(need, 2 * nf * eng.KK0 * 2 * nf)
            need = max(need, 64 * B * 2 * nf)               # up0 dgrad split-K
            if eng.up0_large:                               # cdm_up0_dgrad partials (32768-wide K ranges)
                need = max(need, _cdiv(2 * nf * eng.KK0, 32768) * B * 2 * nf)
        return int(need)
