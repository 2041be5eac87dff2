"""Restatement of the strided (DDIM) sampler on the CPU, independent of cdm_amd: the definition the GPU tests pin it to.

With tau_S = T > ... > tau_1 >= 1, tau_0 = 0 and ab_0 = 1, a step from i = tau_k to j = tau_{k-1}:
    sigma = eta sqrt((1 - ab_j) / (1 - ab_i)) sqrt(1 - ab_i / ab_j)
    cx    = sqrt(ab_j / ab_i)
    ce    = sqrt(1 - ab_j - sigma^2) - sqrt(ab_j (1 - ab_i) / ab_i)
    x_j   = (cx x_i + ce eps) + sigma z                (z = 0 and sigma = 0 when j = 0)
eps = eu + w (ec - eu) with classifier-free guidance.  The coefficients are evaluated in fp64 (python floats) from the
fp32 ab_t table and, for an fp32 run, rounded once to fp32.
"""
import math

import torch


def subsequence(T, S, spacing="uniform"):
    if spacing == "uniform":
        return [int(math.floor(k * T / S + 0.5)) for k in range(1, S + 1)]
    return [max(int(math.ceil(T * (k / S) ** 2)), k) for k in range(1, S + 1)]


def coefficients(ab_t, taus, eta, dtype=torch.float32):
    """(cx, ce, sigma) tensors of S + 1 entries indexed by the position k (entry 0 unused)."""
    ab = [float(v) for v in ab_t.double()]
    ab[0] = 1.0
    cx, ce, sg = [1.0], [0.0], [0.0]
    for k, i in enumerate(taus, start=1):
        j = taus[k - 2] if k > 1 else 0
        s = eta * math.sqrt((1 - ab[j]) / (1 - ab[i])) * math.sqrt(1 - ab[i] / ab[j]) if j else 0.0
        sg.append(s)
        cx.append(math.sqrt(ab[j] / ab[i]))
        ce.append(math.sqrt(1 - ab[j] - s * s) - math.sqrt(ab[j] * (1 - ab[i]) / ab[i]))
    return tuple(torch.tensor(v, dtype=torch.float64).to(dtype) for v in (cx, ce, sg))


def step(x, ec, eu, w, cx, ce, sg, z):
    """One update in separate tensor ops (one rounding each), the order the kernel fixes."""
    eps = ec if eu is None else eu + w * (ec - eu)
    v = cx * x + ce * eps
    if float(sg) != 0.0:
        v = v + sg * z
    return v


def snap(p, S, save_rate):
    """The reference's snapshot rule (code/train_diffusion_condition.py:331) on positions."""
    return p % save_rate == 0 or p == S or p < 8


def sample_loop(model, x, params, guide_w, T, ab_t, taus, eta, save_rate=20):
    """Positions S..1 from x (its dtype is the run's).  CPU-RNG order per position: z (only when eta > 0 and the
    position is not the last), then the shortcut draw(s) inside ``model`` (cond first, then uncond)."""
    dt = x.dtype
    S = len(taus)
    cx, ce, sg = coefficients(ab_t, taus, eta, dt)
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    w = torch.tensor(guide_w, dtype=dt)
    inter = []
    for p in range(S, 0, -1):
        i = taus[p - 1]
        t = torch.tensor([i / T]).to(dt)                   # fp32 value of i / T, as the prologue kernel writes it
        z = torch.randn(x.shape).to(dt) if eta > 0 and p > 1 else None
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
        else:
            ec, eu = model(x, t, params), None
        x = step(x, ec, eu, w, cx[p], ce[p], sg[p], z)
        if snap(p, S, save_rate):
            inter.append(x.clone())
    return x, torch.stack(inter)
