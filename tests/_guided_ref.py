"""Numpy / torch-CPU restatement of observation-guided sampling (diffusion.GuidedDDIMSampler), independent of
cdm_amd: the definition the GPU tests pin the kernels and the sampler to.

Observation model y = A x0 + n, A the f x f block mean, wgt >= 0 per cell (0 = not observed).  At a position with
sq = sqrt(1 - ab_i), ra = 1 / sqrt(ab_i) and the CFG-combined eps = eu + w (ec - eu):
    x0h = (x - sq eps) ra;  m = A x0h (row-major sum of the cell, then * 1 / f^2);  r = y - m
    L[s] = sum_q wgt_q r_q r_q (fp64);  u = A^T-spread of (wgt r) / f^2
    gdir = (-2 ra) u;  ge = (2 sq ra) u;  deps = ge, or w ge on the cond rows and (1 - w) ge on the uncond rows
    grad = gdir + dx_cond (+ dx_uncond),  dx = the network's vector-Jacobian product of deps wrt its image input
    x   <- DDIM step - (zeta / (2 sqrt(L[s]))) grad          nothing subtracted where L[s] == 0 or zeta == 0
In fp32 every line is one rounding, in the order the kernels fix; in fp64 the same expressions with unrounded tables.
"""
import numpy as np
import torch

import _ddim_ref as D


def tables(ab_t, taus, dtype=torch.float32):
    """(sq, ra) tensors of S + 1 entries by position (entry 0: 0, 1), fp64 closed forms from the fp32 ab_t table."""
    ab = [float(v) for v in torch.as_tensor(ab_t).double()]
    sq = [0.0] + [float(np.sqrt(1.0 - ab[i])) for i in taus]
    ra = [1.0] + [float(1.0 / np.sqrt(ab[i])) for i in taus]
    return tuple(torch.tensor(v, dtype=torch.float64).to(dtype) for v in (sq, ra))


def block_mean(v, f):
    """A: [..., H, H] -> [..., H / f, H / f], the cell's pixels added in row-major order, then one product by 1 / f^2."""
    H = v.shape[-1]
    c = v.reshape(*v.shape[:-2], H // f, f, H // f, f)
    s = None
    for a in range(f):
        for b in range(f):
            s = c[..., :, a, :, b] if s is None else s + c[..., :, a, :, b]
    return s * (1.0 / (f * f))


def block_mean_T(q, f):
    """A^T: [..., h, h] -> [..., h f, h f], every pixel of a cell gets the cell's value / f^2."""
    return (q * (1.0 / (f * f))).repeat_interleave(f, -2).repeat_interleave(f, -1)


def fold_sum(terms):
    """The fp64 sum of ``terms`` (1-d) in cdm_obs_residual_grad's order: thread t adds its cells t, t + 256, ... ascending,
    a wave64 butterfly (xor 32, 16, ..., 1), then (w0 + w1) + (w2 + w3)."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    rounds = -(-t.size // 256)
    pad = np.zeros(rounds * 256)
    pad[: t.size] = t
    acc = np.zeros(256)
    for r in pad.reshape(rounds, 256):
        acc = acc + r
    v = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])


def residual_grad(x, ec, eu, w, obs, wgt, f, sq, ra, grads=True, fold=True):
    """The residual / gradient op on x, ec, eu (None without CFG) [n, H, H], obs [n, h, h], wgt [n or 1, h, h]; the dtype
    of x is the run's (fp32: the kernel's roundings; fp64: the same expressions), sq / ra 0-d tensors of that dtype
    holding the table values.  -> dict(L [n] fp64, x0h, and with ``grads``: gdir, ge, deps_c, deps_u)."""
    dt = x.dtype
    n = x.shape[0]
    w = torch.tensor(float(w), dtype=torch.float32).to(dt)
    sq, ra = sq.to(dt), ra.to(dt)
    eps = ec if eu is None else eu + w * (ec - eu)
    x0h = (x - sq * eps) * ra
    m = block_mean(x0h, f)
    wg = wgt.to(dt).expand(n, *wgt.shape[1:])
    seen = wg != 0
    r = torch.where(seen, obs.to(dt) - m, torch.zeros_like(m))           # an unobserved cell's obs is never used
    r64, w64 = r.double(), wg.double()
    terms = (w64 * r64) * r64
    if fold:
        L = torch.tensor([fold_sum(terms[s].reshape(-1).numpy()) for s in range(n)], dtype=torch.float64)
    else:
        L = terms.sum((1, 2))
    out = dict(L=L, x0h=x0h, r=r)
    if grads:
        inv = 1.0 / (f * f)
        u = ((wg * r) * inv).repeat_interleave(f, -2).repeat_interleave(f, -1)
        c_dir = torch.tensor(-2.0 * float(ra), dtype=torch.float64).to(dt)   # formed in fp64, rounded once
        c_eps = torch.tensor(2.0 * float(sq) * float(ra), dtype=torch.float64).to(dt)
        ge = c_eps * u
        out.update(gdir=c_dir * u, ge=ge, deps_c=ge if eu is None else w * ge,
                   deps_u=None if eu is None else (1 - w) * ge)
    return out


def guided_update(x, ec, eu, w, cx, ce, sg, z, gdir, dx_c, dx_u, L, zeta):
    """The DDIM step (tests/_ddim_ref.step) then the guidance step; L [n] fp64; zeta as the kernel receives it (fp32)."""
    dt = x.dtype
    wt = torch.tensor(float(w), dtype=torch.float32).to(dt)
    v = D.step(x, ec, eu, wt, cx, ce, sg, z)
    z32 = float(np.float32(zeta))
    if z32 == 0.0:
        return v
    with np.errstate(divide="ignore"):
        k = z32 / (2.0 * np.sqrt(L.numpy()))
    g = gdir + dx_c
    if dx_u is not None:
        g = g + dx_u
    k = torch.from_numpy(np.where(L.numpy() != 0, k, 0.0)).to(dt).reshape(-1, *([1] * (x.dim() - 1)))
    live = (L != 0).reshape(k.shape)
    return torch.where(live, v - k * g, v)


def closing_L(x, obs, wgt, f):
    """L of x itself (x0h = x, tables sq = 0 and ra = 1); its sqrt is the last row of the misfit history."""
    one, zero = torch.ones((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)
    return residual_grad(x, x, None, 0.0, obs, wgt, f, zero, one, grads=False)["L"]


def trajectory(sd, x_T, params, guide_w, T, ab_t, taus, eta, obs, wgt, f, zeta, rows, zs, dtype, *, n_feat, n_cfeat,
               height, kinks=None, keep=False, npos=None):
    """The guided walk on the oracle's forward (oracle/ref_cpu.py, eval mode) in ``dtype``: x_T [n, H, H] fp32, params
    [n, ncf] or None, rows[S - p] = the shortcut draws of position p ([(w, b)] or [(w, b) cond, (w, b) uncond]), zs[S - p]
    = its z [n, H, H] (None where none is drawn).  The image gradient is autograd's.  kinks: None, or kinks(p, half) -> a
    context manager entered around the forward of half 0 (cond) / 1 (uncond) of position p (tests/_kinks.Kinks).
    npos: stop after that many positions (the closing row then belongs to the state reached).
    -> (x, misfit [positions + 1, n] fp64, per-position records when ``keep``)."""
    from oracle import ref_cpu as R
    S = len(taus)
    cx, ce, sg = D.coefficients(ab_t, taus, eta, dtype)
    sq, ra = tables(ab_t, taus, dtype)
    cfg = guide_w > 0 and params is not None
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x = x_T.to(dtype)
    n = x.shape[0]
    c = params.to(dtype) if params is not None else None
    hist, rec = [], []

    def fwd(xin, cc, sc, p, half):
        ctx = kinks(p, half) if kinks is not None else None
        if ctx is not None:
            ctx.__enter__()
        try:
            return R.unet_forward(sd, xin[:, None], tin, cc, n_feat=n_feat, n_cfeat=n_cfeat, height=height, train=False,
                                  shortcut=(sc[0].to(dtype), sc[1].to(dtype)))[:, 0]
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)

    for p in range(S, S - (S if npos is None else npos), -1):
        tin = torch.tensor([taus[p - 1] / T]).to(dtype)              # the fp32 value of i / T, as the prologue writes it
        sc = rows[S - p]
        xin = x.detach().clone().requires_grad_(True)
        ec = fwd(xin, c, sc[0], p, 0)
        eu = fwd(xin, torch.zeros_like(c), sc[1], p, 1) if cfg else None
        o = residual_grad(x, ec.detach(), None if eu is None else eu.detach(), guide_w, obs, wgt, f, sq[p], ra[p])
        hist.append(o["L"])
        dx_c = dx_u = None
        if float(np.float32(zeta)) != 0.0:
            dx_c = torch.autograd.grad((ec * o["deps_c"]).sum(), xin, retain_graph=cfg)[0]
            if cfg:
                dx_u = torch.autograd.grad((eu * o["deps_u"]).sum(), xin)[0]
        if keep:
            grad = None if dx_c is None else (o["gdir"] + dx_c if dx_u is None else o["gdir"] + dx_c + dx_u)
            rec.append(dict(p=p, x=x.clone(), tin=tin, L=o["L"], grad=grad))
        x = guided_update(x, ec.detach(), None if eu is None else eu.detach(), guide_w, cx[p], ce[p], sg[p], zs[S - p],
                          o.get("gdir"), dx_c, dx_u, o["L"], zeta).detach()
    hist.append(closing_L(x, obs, wgt, f))
    misfit = torch.stack(hist).sqrt()
    return (x, misfit, rec) if keep else (x, misfit)
