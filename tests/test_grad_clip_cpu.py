"""Host side of global-norm gradient clipping: trainer.clip_coef against torch.nn.utils.clip_grad_norm_.

clip_coef restates what the device computes, float32(min(1, max_norm / (norm + 1e-6))) with the quotient in fp64.
torch evaluates the same quotient in fp32 from an fp32 norm: the norm carries a relative error of a few 2^-24 (the
square root and the sum over the per-parameter norms), the add of 1e-6 and the division one rounding each.  The factor
inferred from torch's scaled gradients adds the rounding of the product g * coef read back through a division by g,
2^-24 relative each.  8 * 2^-24 relative covers the chain; where clipping is off both give exactly 1.
"""
import math
import struct

import pytest
import torch

from cdm_amd import _lib
from cdm_amd.trainer import clip_coef

U = 2.0 ** -24


def _grads(seed, sizes=(1000, 37, 4096, 1)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes]


def _norm64(gs):
    return math.sqrt(math.fsum(float(x) * float(x) for t in gs for x in t.tolist()))


@pytest.mark.parametrize("case", ["below", "above", "at"])
def test_clip_coef_matches_torch_clip_grad_norm(case):
    gs = _grads(3)
    norm = _norm64(gs)
    # "at": max_norm within 1e-6 of the norm, where the + 1e-6 of the denominator decides whether clipping is on
    max_norm = {"below": 2.0 * norm, "above": 0.25 * norm, "at": norm + 5e-7}[case]
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in gs]
    for p, t in zip(params, gs):
        p.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert abs(float(total) - norm) <= 8 * U * norm
    want = clip_coef(norm, max_norm)
    assert want == struct.unpack("f", struct.pack("f", want))[0], "clip_coef returns an fp32 value"
    assert want == struct.unpack("f", struct.pack("f", min(1.0, max_norm / (norm + 1e-6))))[0]
    big = max(range(len(gs)), key=lambda i: gs[i].numel())
    k = int(gs[big].abs().argmax())
    inferred = float(params[big].grad[k].double() / gs[big][k].double())
    print(f"{case}: norm {norm:.9g} max_norm {max_norm:.9g} clip_coef {want:.9g} torch {inferred:.9g}")
    assert abs(inferred - want) <= 8 * U * want
    if case == "below":
        assert want == 1.0 and all(torch.equal(p.grad, t) for p, t in zip(params, gs))
    if case == "above":
        assert want < 0.26
    if case == "at":
        assert 0.0 <= 1.0 - want < 1e-6               # the quotient is 1 - 5e-7 / norm: fp32 may round it to 1


def test_clip_coef_special_values():
    assert clip_coef(123.456, float("inf")) == 1.0
    assert clip_coef(0.0, float("inf")) == 1.0
    assert clip_coef(0.0, 1e-3) == 1.0                # a zero gradient is never scaled up: min(1, 1e-3 / 1e-6)
    assert clip_coef(1e30, 1.0) == struct.unpack("f", struct.pack("f", 1.0 / (1e30 + 1e-6)))[0]
    assert clip_coef(2.0, 1.0) == struct.unpack("f", struct.pack("f", 1.0 / 2.000001))[0]


def test_header_prototypes_of_the_clipped_step():
    import ctypes
    protos = _lib.parse_header()
    vp, ll, i, d, f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_float
    assert protos["cdm_grad_sumsq"] == [vp, ll, vp, vp, vp]
    ema = list(protos["cdm_adam_ema"])
    # cdm_adam_ema's list with max_norm, partial, clip_rec, skipped in front of the stream
    assert protos["cdm_adam_clipped"] == ema[:-1] + [vp, vp, vp, vp] + ema[-1:]
    assert protos["cdm_adam"] == [vp, vp, vp, vp, ll, vp, vp, i, d, d, d, f, vp]
    import re
    from cdm_amd.trainer import GRAD_SUMSQ_MAX_PARTIALS
    m = re.search(r"#define\s+CDM_GRAD_SUMSQ_MAX_PARTIALS\s+(\d+)", open(_lib.HEADER).read())
    assert m and int(m.group(1)) == GRAD_SUMSQ_MAX_PARTIALS, "the trainer's slab size follows the header"


def test_trainer_rejects_bad_thresholds_before_touching_the_model():
    from cdm_amd.trainer import Trainer
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            Trainer(None, 1e-3, 10, 4, clip_grad_norm=bad)
