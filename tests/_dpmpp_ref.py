"""Restatement of the multistep (DPM-Solver++ 2M) sampler on the CPU, independent of cdm_amd: the definition the GPU
tests pin it to.

With tau_S = T > ... > tau_1 >= 1, tau_0 = 0 and ab_0 = 1, alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha /
sigma), a step from i = tau_k to j = tau_{k-1} with h_k = lambda_j - lambda_i (h_1 = +inf: cx[1] = 0, cd[1] = 1):
    sq = sigma_i,  ra = 1 / alpha_i,  cx = sigma_j / sigma_i,  cd = alpha_j - sigma_j alpha_i / sigma_i
    order 2 and 1 < k < S:  r = h_{k+1} / h_k,  c0 = 1 + 1 / (2 r),  c1 = -1 / (2 r);    otherwise c0 = 1, c1 = 0
    d   = (x_i - sq eps) ra
    D   = d if c1 == 0 else c0 d + c1 d_prev
    x_j = cx x_i + cd D ;   d_prev <- d
eps = eu + w (ec - eu) with classifier-free guidance.  The coefficients are evaluated in fp64 (python floats) from the
fp32 ab_t table and, for an fp32 run, rounded once to fp32.
"""
import math

import torch

from _ddim_ref import snap, subsequence  # noqa: F401  (the same positions and snapshot rule)


def coefficients(ab_t, taus, order=2, dtype=torch.float32):
    """(sq, ra, c0, c1, cx, cd) tensors of S + 1 entries indexed by the position k (entry 0 unused)."""
    ab = [float(v) for v in ab_t.double()]
    ab[0] = 1.0
    S = len(taus)
    tau = [0] + list(taus)
    lam = [math.inf] + [math.log(math.sqrt(ab[i]) / math.sqrt(1 - ab[i])) for i in taus]      # lambda at tau_0..tau_S
    h = [None] + [lam[k - 1] - lam[k] for k in range(1, S + 1)]
    sq, ra, c0, c1, cx, cd = [0.0], [1.0], [1.0], [0.0], [1.0], [0.0]
    for k in range(1, S + 1):
        i, j = tau[k], tau[k - 1]
        al_i, al_j, sg_i, sg_j = math.sqrt(ab[i]), math.sqrt(ab[j]), math.sqrt(1 - ab[i]), math.sqrt(1 - ab[j])
        sq.append(sg_i)
        ra.append(1 / al_i)
        cx.append(sg_j / sg_i)
        cd.append(al_j - sg_j * al_i / sg_i)
        if order == 2 and 1 < k < S:
            r = h[k + 1] / h[k]
            c0.append(1 + 1 / (2 * r))
            c1.append(-1 / (2 * r))
        else:
            c0.append(1.0)
            c1.append(0.0)
    return tuple(torch.tensor(v, dtype=torch.float64).to(dtype) for v in (sq, ra, c0, c1, cx, cd))


def step(x, ec, eu, w, sq, ra, c0, c1, cx, cd, d_prev):
    """One update in separate tensor ops (one rounding each), the order the kernel fixes -> (x_new, d).  d_prev is not
    touched where c1 == 0."""
    eps = ec if eu is None else eu + w * (ec - eu)
    d = (x - sq * eps) * ra
    D = d if float(c1) == 0.0 else c0 * d + c1 * d_prev
    return cx * x + cd * D, d


def sample_loop(model, x, params, guide_w, T, taus, tables, save_rate=20):
    """Positions S..1 from x (its dtype is the run's; ``tables`` = (sq, ra, c0, c1, cx, cd), arrays or tensors, are cast
    to it, so an fp32 and an fp64 run share one set).  CPU-RNG order per position: the shortcut draw(s) inside ``model``
    (cond first, then uncond), nothing else.  Snapshots as _ddim_ref.sample_loop."""
    dt = x.dtype
    S = len(taus)
    sq, ra, c0, c1, cx, cd = (torch.as_tensor(v).to(dt) for v in tables)
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    w = torch.tensor(guide_w, dtype=dt)
    d_prev = None
    inter = []
    for p in range(S, 0, -1):
        i = taus[p - 1]
        t = torch.tensor([i / T]).to(dt)                   # fp32 value of i / T, as the prologue kernel writes it
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
        else:
            ec, eu = model(x, t, params), None
        x, d_prev = step(x, ec, eu, w, sq[p], ra[p], c0[p], c1[p], cx[p], cd[p], d_prev)
        if snap(p, S, save_rate):
            inter.append(x.clone())
    return x, torch.stack(inter)
