"""Restatement of masked (inpainting) sampling on the CPU, independent of cdm_amd: the definition the GPU tests pin it to.

After every sampler step that takes the state from timestep i to timestep j (j = i - 1 for the ancestral sampler,
j = tau_{k-1} for the strided ones, j = 0 after the last step), with m the mask (1 = known pixel) and xi standard normal:
    kn  = sab[j] known + somab[j] xi        for j >= 1        sab = sqrt(ab), somab = sqrt(1 - ab)
    kn  = known                             for j == 0        (no xi, no multiply)
    x_j = m kn + (1 - m) x_j                each product and the sum one rounding; m == 1 gives kn and m == 0 gives x_j
                                            as they are (bit for bit, whatever the other operand holds)
sab / somab are evaluated in fp64 (python floats) from the fp32 ab_t table and, for an fp32 run, rounded once to fp32.
xi is one draw for the whole run ("fixed") or one per step with j >= 1 ("fresh").  The starting x_T is not blended.

CPU-RNG order of the loops: "fixed", xi once before the loop; per position z (if the sampler draws one there), then the
"fresh" xi (only where j >= 1), then the shortcut draw(s) inside ``model`` (cond first, then uncond).

The three loops are those of oracle/ref_cpu.py (ancestral), tests/_ddim_ref.py and tests/_dpmpp_ref.py with the blend
after the step; their step functions are used unchanged.
"""
import math

import torch

import _ddim_ref as D
import _dpmpp_ref as P


def tables(ab_t, dtype=torch.float32):
    """(sab, somab) tensors of T + 1 entries indexed by the timestep; entry 0 is (1, 0) exactly."""
    ab = [float(v) for v in ab_t.double()]
    ab[0] = 1.0
    sab = torch.tensor([math.sqrt(a) for a in ab], dtype=torch.float64)
    somab = torch.tensor([math.sqrt(1 - a) for a in ab], dtype=torch.float64)
    return sab.to(dtype), somab.to(dtype)


def blend(x, known, mask, sab_j, somab_j, xi, j):
    """The blend in separate tensor ops (one rounding each).  ``mask`` broadcasts over the batch; xi is not touched
    when j == 0 (it may be None)."""
    if j >= 1:
        kn = sab_j * known + somab_j * xi
    else:
        kn = known
    a = mask * kn
    b = (1 - mask) * x
    v = a + b
    v = torch.where(mask == 1, kn, v)
    return torch.where(mask == 0, x, v)


def _draw(x):
    return torch.randn(x.shape).to(x.dtype)          # an fp32 draw, cast: the fp64 run sees the identical numbers


class _Blender:
    """The per-run state of the blend inside a loop: tables in the run's dtype, the "fixed" xi, the draw order."""

    def __init__(self, x, ab_t, known, mask, mode):
        assert mode in ("fixed", "fresh")
        self.mode = mode
        self.known, self.mask = known.to(x.dtype), mask.to(x.dtype)
        self.sab, self.somab = tables(ab_t, x.dtype)
        self.xi = _draw(x) if mode == "fixed" else None          # before the loop

    def draw(self, x, j):
        """Called at every position after its z and before the model: the "fresh" draw."""
        if self.mode == "fresh" and j >= 1:
            self.xi = _draw(x)

    def __call__(self, x, j):
        return blend(x, self.known, self.mask, self.sab[j], self.somab[j], self.xi, j)


def ancestral_loop(model, x, params, guide_w, T, sched, known, mask, mode, save_rate=20):
    """oracle/ref_cpu.sample_loop (denoise_add_noise, code/train_diffusion_condition.py:274-279) with the blend after
    every step; ``sched`` = (b_t, a_t, ab_t) in the run's dtype except that the blend tables always come from the fp32
    ab_t values they hold."""
    from oracle import ref_cpu as R
    b_t, a_t, ab_t = sched
    dt = x.dtype
    bl = _Blender(x, ab_t.float(), known, mask, mode)
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    inter = []
    for i in range(T, 0, -1):
        t = torch.tensor([i / T]).to(dt)
        z = _draw(x) if i > 1 else 0
        bl.draw(x, i - 1)
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
            eps = eu + guide_w * (ec - eu)
        else:
            eps = model(x, t, params)
        x = R.denoise_add_noise(x, i, eps, z, b_t, a_t, ab_t)
        x = bl(x, i - 1)
        if i % save_rate == 0 or i == T or i < 8:
            inter.append(x.clone())
    return x, torch.stack(inter)


def ddim_loop(model, x, params, guide_w, T, ab_t, taus, eta, known, mask, mode, save_rate=20):
    """tests/_ddim_ref.sample_loop with the blend after every position."""
    dt = x.dtype
    S = len(taus)
    cx, ce, sg = D.coefficients(ab_t, taus, eta, dt)
    bl = _Blender(x, ab_t, known, mask, mode)
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    w = torch.tensor(guide_w, dtype=dt)
    inter = []
    for p in range(S, 0, -1):
        i, j = taus[p - 1], (taus[p - 2] if p > 1 else 0)
        t = torch.tensor([i / T]).to(dt)
        z = _draw(x) if eta > 0 and p > 1 else None
        bl.draw(x, j)
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
        else:
            ec, eu = model(x, t, params), None
        x = D.step(x, ec, eu, w, cx[p], ce[p], sg[p], z)
        x = bl(x, j)
        if D.snap(p, S, save_rate):
            inter.append(x.clone())
    return x, torch.stack(inter)


def dpmpp_loop(model, x, params, guide_w, T, ab_t, taus, tabs, known, mask, mode, save_rate=20):
    """tests/_dpmpp_ref.sample_loop with the blend after every position (``tabs`` = (sq, ra, c0, c1, cx, cd), cast to
    the run's dtype as there); d_prev is the data prediction computed before the blend."""
    dt = x.dtype
    S = len(taus)
    sq, ra, c0, c1, cx, cd = (torch.as_tensor(v).to(dt) for v in tabs)
    bl = _Blender(x, ab_t, known, mask, mode)
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    w = torch.tensor(guide_w, dtype=dt)
    d_prev = None
    inter = []
    for p in range(S, 0, -1):
        i, j = taus[p - 1], (taus[p - 2] if p > 1 else 0)
        t = torch.tensor([i / T]).to(dt)
        bl.draw(x, j)
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
        else:
            ec, eu = model(x, t, params), None
        x, d_prev = P.step(x, ec, eu, w, sq[p], ra[p], c0[p], c1[p], cx[p], cd[p], d_prev)
        x = bl(x, j)
        if D.snap(p, S, save_rate):
            inter.append(x.clone())
    return x, torch.stack(inter)
