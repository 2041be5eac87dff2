"""Torch-CPU / numpy restatement of the parameter fit's definition (likelihood.ParamFit) on the oracle's forward.

Positions, noise and shortcut rows are the scan's (tests/_scan_ref.py).  One evaluation at parameters c [M, K, ncf]:
    x_p[m]     = sab[t_p] x[m] + omab[t_p] z_p[m]                    fp32, the same values in the fp32 and the fp64 run
    eps_p[m,k] = unet_forward(eval)(x_p[m], t_p / T, c[m,k])          in ``dtype``, batch row m K + k
    score[m,k] = (1 / R) sum_p w[t_p] mean_pixels (eps_p - z_p)^2     the difference in ``dtype``, squares and sums fp64
    deps_p     = coef_p (eps_p - z_p),  coef_p = 2 w[t_p] / (H W R)   fp64 run: exact; fp32 run: coef rounded to fp32 once
    g[m,k,:]   = sum_p dc_p[m,k,:]                                     dc_p = autograd of sum(eps_p * deps_p) wrt c in
                                                                       ``dtype``; the sum over p in fp64, p ascending
``update`` restates cdm_fit_update in numpy fp64, one IEEE operation per numpy call in the kernel's order, and ``fit``
runs the whole loop (pass n = 1..iters: evaluate, record, track the best, update; pass iters + 1: evaluate and record).
The network input of every pass is c32 = (float) c64, as on the device."""
import numpy as np
import torch

from oracle import ref_cpu as R
import _scan_ref as SR


def evaluate(sd, x, c, T, t_grid, n_noise, noise, rows, dtype, kind="uniform", *, n_feat, n_cfeat, height, kinks=None,
             per_position=False):
    """-> (score [M, K] fp64, g [M, K, ncf] fp64).  x [M,H,H] fp32, c [M,K,ncf] (any float dtype: cast to ``dtype``),
    noise [P,M,H,H] fp32, rows = _scan_ref.draw_rows(...).  kinks: None, or kinks(p) -> a context manager entered
    around position p's forward (tests/_kinks.Kinks: capture or impose the ReLU / MaxPool decisions).
    per_position: also return the list of dc_p [M,K,ncf] (``dtype``)."""
    _, _, ab_t = R.make_schedule(T)
    sab, omab = ab_t.sqrt(), 1 - ab_t
    w = SR.weights(kind, T)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    M, K, ncf = c.shape
    S, HW = len(t_grid), height * height
    P = S * n_noise
    assert noise.shape == (P, M, height, height) and len(rows) == P
    score = torch.zeros(M, K, dtype=torch.float64)
    g = torch.zeros(M, K, ncf, dtype=torch.float64)
    dcs = []
    for p in range(P):
        t = t_grid[p % S]
        z = noise[p]
        xp = sab[t] * x + omab[t] * z                                   # fp32, two products and a sum
        tin = torch.tensor([t / T])                                      # fp32 rounding of the fp64 quotient
        sw, sb = rows[p]
        cc = c.reshape(M * K, ncf).to(dtype).clone().requires_grad_(True)
        xin = xp[:, None].repeat_interleave(K, 0).to(dtype)             # row m K + k = map m
        zz = z.repeat_interleave(K, 0).to(dtype)
        ctx = kinks(p) if kinks is not None else None
        if ctx is not None:
            ctx.__enter__()
        try:
            eps = R.unet_forward(sd, xin, tin.to(dtype), cc, n_feat=n_feat, n_cfeat=n_cfeat, height=height,
                                 train=False, shortcut=(sw.to(dtype), sb.to(dtype)))
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        d = (eps[:, 0] - zz).detach()
        d64 = d.double()
        mse = (d64 * d64).sum((1, 2)) / HW
        score += (w[t] * mse / n_noise).reshape(M, K)
        coef = 2.0 * w[t].item() / n_noise / HW
        if dtype == torch.float32:
            coef = float(np.float32(coef))
        (eps[:, 0] * (coef * d)).sum().backward()
        dcs.append(cc.grad.reshape(M, K, ncf).clone())
        g += dcs[-1].double()
    return (score, g, dcs) if per_position else (score, g)


def bias_table(beta1, beta2, iters):
    """[iters, 2] fp64: 1 - beta1**n, 1 - beta2**n for n = 1..iters (Python floats, as likelihood.fit_bias_table)."""
    return np.array([(1 - beta1 ** float(n), 1 - beta2 ** float(n)) for n in range(1, iters + 1)],
                    dtype=np.float64).reshape(iters, 2)


def new_state(c32, iters):
    """The optimiser state of rows = c32.shape[0] starts, as _FitRun.load leaves it."""
    c32 = np.ascontiguousarray(c32, dtype=np.float32)
    rows, ncf = c32.shape
    return dict(done=0, c32=c32.copy(), c64=c32.astype(np.float64), m=np.zeros((rows, ncf)), v=np.zeros((rows, ncf)),
                best_score=np.full(rows, np.inf), best_c=c32.copy(), stalled=np.zeros(rows, dtype=np.int32),
                hist_score=np.full((iters + 1, rows), np.nan), hist_gnorm=np.full((iters + 1, rows), np.nan))


def update(st, score, g, iters, free, lo, hi, lr, beta1, beta2, eps, bc):
    """cdm_fit_update on the state dict ``st`` (in place): score [rows] fp64, g [rows, ncf] fp64, free [ncf] 0/1, lo /
    hi [ncf] fp64, bc = bias_table(...).  Every line is one IEEE fp64 operation per element, in the kernel's order."""
    n0 = st["done"]
    if n0 < 0 or n0 > iters:
        return
    score, g = np.asarray(score, dtype=np.float64), np.asarray(g, dtype=np.float64)
    rows, ncf = g.shape
    fr = [j for j in range(ncf) if free[j]]
    with np.errstate(all="ignore"):
        ss = np.zeros(rows)
        finite = np.isfinite(score)
        for j in fr:
            finite &= np.isfinite(g[:, j])
            ss = ss + g[:, j] * g[:, j]
        st["hist_score"][n0] = score
        st["hist_gnorm"][n0] = np.sqrt(ss)
        better = score < st["best_score"]
        st["best_c"][better] = st["c32"][better]
        if n0 < iters:
            st["stalled"][~finite] += 1
            omb1, omb2 = 1.0 - beta1, 1.0 - beta2
            bc1, bc2 = bc[n0]
            for j in fr:
                gj = g[:, j]
                m1 = beta1 * st["m"][:, j] + omb1 * gj
                v1 = beta2 * st["v"][:, j] + omb2 * (gj * gj)
                mhat, vhat = m1 / bc1, v1 / bc2
                step = (lr * mhat) / (np.sqrt(vhat) + eps)
                c = st["c64"][:, j] - step
                c = np.where(c < lo[j], lo[j], np.where(c > hi[j], hi[j], c))
                for name, val in (("m", m1), ("v", v1), ("c64", c)):
                    st[name][:, j] = np.where(finite, val, st[name][:, j])
                st["c32"][:, j] = np.where(finite, c.astype(np.float32), st["c32"][:, j])
        st["best_score"] = np.where(better, score, st["best_score"])
    st["done"] = n0 + 1


def fit(sd, x, start, T, t_grid, n_noise, noise, rows, dtype, iters, lr, free=None, bounds=(0.0, 1.0),
        betas=(0.9, 0.999), eps=1e-8, kind="uniform", *, n_feat, n_cfeat, height):
    """The whole fit with the network in ``dtype``: start [M,K,ncf] fp32 -> the final state dict of ``update`` (arrays
    over rows = M K, row m K + k), plus "g" = the list of the iters + 1 gradients [M,K,ncf]."""
    M, K, ncf = start.shape
    mask = np.ones(ncf, dtype=np.int32) if free is None else np.isin(np.arange(ncf), free).astype(np.int32)
    lo, hi = (np.broadcast_to(np.asarray(b, dtype=np.float64), (ncf,)) for b in bounds)
    bc = bias_table(betas[0], betas[1], iters)
    st = new_state(start.reshape(M * K, ncf).numpy(), iters)
    st["g"] = []
    for _ in range(iters + 1):
        c = torch.from_numpy(st["c32"].copy()).reshape(M, K, ncf)
        score, g = evaluate(sd, x, c, T, t_grid, n_noise, noise, rows, dtype, kind, n_feat=n_feat, n_cfeat=n_cfeat,
                            height=height)
        st["g"].append(g.numpy().copy())
        update(st, score.reshape(-1).numpy(), g.reshape(M * K, ncf).numpy(), iters, mask, lo, hi, lr, betas[0],
               betas[1], eps, bc)
    return st
