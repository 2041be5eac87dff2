"""Symmetry augmentation of square single-channel maps: the dihedral group D4 and periodic shifts.

The fields are projections of periodic, statistically isotropic boxes and the conditioning parameters are scalars, so
flips, quarter turns and periodic rolls are exact symmetries of the data distribution.  An op for one sample is three
integers ``(g, dy, dx)``, ``g`` in 0..7 and ``dy``, ``dx`` in 0..H-1: ``f = g >> 2`` flips the columns, then
``r = g & 3`` quarter turns, then a roll, which on one ``[H, H]`` map ``x`` is

    x = x.flip(-1) if f else x
    x = torch.rot90(x, r, (-2, -1))
    x = torch.roll(x, (dy, dx), (-2, -1))

A pure gather (every output pixel is one input pixel), so results are bit-exact.  Output pixel (i, j) is input pixel
(i', j'); with n = H - 1, a = (i - dy) mod H, b = (j - dx) mod H:

    g   0   1      2      3      4      5   6      7
    i'  a   b      n - a  n - b  a      b   n - a  n - b
    j'  b   n - a  n - b  a      n - b  a   b      n - a

The gather runs on the device (csrc/misc.hip: ``cdm_perturb_aug``, folded into the training step's perturb kernel);
the ops of a training step are drawn there too (``cdm_augment_draw``), from the step's Philox counter.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import lib

MODES = {"none": 0, "d4": 1, "shift": 2, "d4+shift": 3}     # cdm_augment_draw's mode: bit 0 draws g, bit 1 dy and dx


def check_mode(mode) -> int:
    """The integer ``cdm_augment_draw`` takes for ``mode``; ValueError for anything but the four names."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"augment must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


def augment_source_index(H: int, g: int, dy: int, dx: int) -> np.ndarray:
    """Flat gather index of the op, int64 ``[H * H]``: ``out.reshape(-1) == x.reshape(-1)[index]`` (host only)."""
    H, g, dy, dx = int(H), int(g), int(dy), int(dx)
    if H < 1 or not 0 <= g <= 7 or not 0 <= dy < H or not 0 <= dx < H:
        raise ValueError(f"op (g={g}, dy={dy}, dx={dx}) outside g in 0..7, dy, dx in 0..{H - 1}")
    n = H - 1
    i, j = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(H, dtype=np.int64), indexing="ij")
    a, b = (i - dy) % H, (j - dx) % H
    si, sj = ((a, b), (b, n - a), (n - a, n - b), (n - b, a))[g & 3]
    if g & 4:
        sj = n - sj
    return (si * H + sj).reshape(-1)


def check_augment_ops(ops, B: int, H: int) -> torch.Tensor:
    """``ops`` as the int32 ``[B, 3]`` tensor the kernels read.  ValueError unless it is an integer tensor of that
    shape with g in 0..7 and dy, dx in 0..H-1 (reads the values on the host: one sync when ``ops`` is on the device)."""
    if not isinstance(ops, torch.Tensor):
        raise ValueError(f"aug_ops must be an integer tensor [B, 3], got {type(ops).__name__}")
    if ops.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"aug_ops must be int32 or int64, got {ops.dtype}")
    if tuple(ops.shape) != (int(B), 3):
        raise ValueError(f"aug_ops must have shape [{int(B)}, 3], got {list(ops.shape)}")
    host = ops.detach().cpu()
    if B and (int(host.min()) < 0 or int(host[:, 0].max()) > 7 or int(host[:, 1:].max()) > int(H) - 1):
        raise ValueError(f"aug_ops out of range: g must lie in 0..7 and dy, dx in 0..{int(H) - 1}")
    return ops.to(torch.int32).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def augment_maps(x: torch.Tensor, ops: torch.Tensor) -> torch.Tensor:
    """Apply one op per map on the device.  ``x`` ``[B, 1, H, H]`` or ``[B, H, H]`` fp32, ``ops`` integer ``[B, 3]``;
    returns a new tensor of x's shape."""
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1) or x.shape[-1] != x.shape[-2]:
        raise ValueError(f"expected maps of shape [B, 1, H, H] or [B, H, H], got {list(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"expected fp32 maps, got {x.dtype}")
    if x.device.type != "cuda":
        raise RuntimeError("augment_maps runs on the MI355X HIP kernels: move the maps to a cuda device")
    B, H = x.shape[0], x.shape[-1]
    o = check_augment_ops(ops, B, H).to(x.device)
    x = x.contiguous()
    out = torch.empty_like(x)
    if B:
        lib().cdm_perturb_aug(_p(x), _p(o), None, None, None, 0, None, None, B, H * H, H, 0, _p(out), None, _s())
    return out


def draw_augment_ops(B: int, H: int, mode: str, seed: int, sub: int = 0, device="cuda") -> torch.Tensor:
    """The ops the device draws for ``(seed, sub)``: int32 ``[B, 3]`` on the device (the Trainer's step k draws
    ``sub = (4 << 24) + k`` with its own per-rank seed)."""
    m = check_mode(mode)
    if int(B) < 1 or int(H) < 1:
        raise ValueError(f"B and H must be >= 1, got B={B}, H={H}")
    ops = torch.empty(int(B), 3, dtype=torch.int32, device=device)
    lib().cdm_augment_draw(_p(ops), int(B), int(H), m, int(seed), int(sub), None, _s())
    return ops
