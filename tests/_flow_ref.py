"""Numpy / torch-CPU restatement of DDIM encoding and the flow likelihood (diffusion.DDIMEncoder and
diffusion.FlowLikelihood), independent of cdm_amd: the definition the tests pin the tables, the kernels and the drivers to.

With taus = tau_1 < ... < tau_S = T, tau_0 = 0, ab_0 = 1 and (cx_k, ce_k) the eta = 0 DDIM coefficients of the sampler
step tau_k -> tau_{k-1} (tests/_ddim_ref.coefficients), the encoding step k = 1..S takes the state from tau_{k-1} to tau_k:
    eps = eps_theta(x, tau_k, c);   x <- ix_k x + ie_k eps,   ix_k = 1 / cx_k,  ie_k = -ce_k / cx_k
Its Jacobian is ix_k (I + g_k J_k), g_k = -ce_k, J_k = d eps / d x, so with D = H H and q_k = v^T J_k v (a Rademacher
probe v; q_k = tr J_k in expectation)
    log p(x_0 | c) = log N(x_T; 0, I) + (D / 2) log ab_T + sum_k ld_k
    ld_k = g_k q_k ("trace")   or   D log1p(g_k q_k / D) ("logdet"; NaN where 1 + g_k q_k / D <= 0)
In fp32 the update is two products and a sum, each one rounding; the fp64 lines (q, ld, the sums) are one rounding each,
in the order the kernels fix.
"""
import math

import numpy as np
import torch

from _guided_ref import fold_sum

LOG_2PI = 1.83787706640934548356
LN2 = 0.69314718055994530942
FORMS = ("trace", "logdet")          # the kernel's form argument is the index


def _splitmix64(x):
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def run_key(seed, r):
    """The run key of probe run r under ``seed``: splitmix64(splitmix64(seed) + r mod 2^64)."""
    return _splitmix64((_splitmix64(seed & ((1 << 64) - 1)) + r) & ((1 << 64) - 1))


def coefficients(ab_t, taus, dtype=torch.float32):
    """(ix, ie in ``dtype``, g fp64) tensors of S + 1 entries indexed by the step k (entry 0: 1, 0, 0), python-float
    closed forms from the fp32 ab_t table."""
    ab = [float(v) for v in torch.as_tensor(ab_t).double()]
    ab[0] = 1.0
    ix, ie, g = [1.0], [0.0], [0.0]
    for k, i in enumerate(taus, start=1):
        j = taus[k - 2] if k > 1 else 0
        cx = math.sqrt(ab[j] / ab[i])
        ce = math.sqrt(1 - ab[j]) - math.sqrt(ab[j] * (1 - ab[i]) / ab[i])
        ix.append(1 / cx); ie.append(-ce / cx); g.append(-ce)
    t = lambda v, dt: torch.tensor(v, dtype=torch.float64).to(dt)    # noqa: E731
    return t(ix, dtype), t(ie, dtype), t(g, torch.float64)


def probe_from_uniform(u):
    """The Rademacher probe of a position from the uniforms of its Philox stream: +1 where u < 0.5, else -1 (fp32)."""
    u = torch.as_tensor(u)
    return torch.where(u < 0.5, torch.ones_like(u), -torch.ones_like(u))


def log1p_ieee(a):
    """cdm_flow_step's log(1 + a), a > -1, from IEEE operations alone, line by line (csrc/flow.hip, log1p_ieee): frexp
    with the mantissa moved into [sqrt(1/2), sqrt 2), s = a / (2 + a) where the exponent is 0 and (m - 1) / (m + 1)
    otherwise, the atanh series in z = s^2 up to z^11 / 23 by Horner, e ln2 + 2 s h."""
    a = np.float64(a)
    y = np.float64(1.0) + a
    m, e = np.frexp(y)
    m, e = np.float64(m), int(e)
    if m < 0.70710678118654752440:
        m = m * np.float64(2.0)
        e -= 1
    s = a / (np.float64(2.0) + a) if e == 0 else (m - np.float64(1.0)) / (m + np.float64(1.0))
    z = s * s
    h = np.float64(1.0) / np.float64(23.0)
    for k in range(21, 0, -2):
        h = h * z + np.float64(1.0) / np.float64(k)
    r = (np.float64(2.0) * s) * h
    return np.float64(e) * np.float64(LN2) + r


def ld_term(gq, D, form):
    """ld of one row from g q (fp64): "trace" g q; "logdet" D log1p_ieee((g q) / D) where that argument is > -1, else
    NaN."""
    gq = np.float64(gq)
    if form == "trace":
        return gq
    with np.errstate(invalid="ignore", over="ignore"):
        r = gq / np.float64(D)
        return np.float64(D) * log1p_ieee(r) if r > -1.0 else np.float64("nan")


def flow_step(x, eps, dx, v, ix, ie, g, form, acc):
    """cdm_flow_step on x, eps, dx [n, H, H] fp32 and the probe v [H, H] fp32; ix, ie 0-d fp32 tensors, g a python float
    (the fp64 table value), acc [n] fp64 numpy.  -> (x_new fp32, q [n] fp64, acc_new [n] fp64, invalid [n] bool)."""
    n = x.shape[0]
    D = x[0].numel()
    v64 = v.double().reshape(-1).numpy()
    q = np.array([fold_sum(dx[s].double().reshape(-1).numpy() * v64) for s in range(n)], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ld = np.array([ld_term(np.float64(g) * q[s], D, form) for s in range(n)], dtype=np.float64)
        acc_new = acc + ld
    return ix * x + ie * eps, q, acc_new, ~np.isfinite(ld)


def finish(x, log_abT, acc):
    """cdm_flow_finish: (prior [n], logp [n]) fp64 numpy from x [n, H, H] fp32, in the kernel's summation order."""
    n = x.shape[0]
    hD = np.float64(0.5) * np.float64(x[0].numel())
    ss = np.array([fold_sum(x[s].double().reshape(-1).numpy() ** 2) for s in range(n)], dtype=np.float64)
    prior = np.float64(-0.5) * ss - hD * np.float64(LOG_2PI)
    return prior, (prior + hD * np.float64(log_abT)) + acc


def vjp_q(eps, xin, v):
    """q = v^T J v per row by autograd: J = d eps / d xin [n, H, H], v [H, H] (shared by the rows) -> (q [n], dx)."""
    dx = torch.autograd.grad((eps * v.to(eps.dtype)).sum(), xin)[0]
    return (dx * v.to(dx.dtype)).flatten(1).sum(1), dx


def walk(eps_fn, x0, ab_t, taus, dtype, vs=None, form="logdet", npos=None, tables=None):
    """The ascending walk in ``dtype`` from x0 [n, H, H]: ``eps_fn(x, k)`` is the network at the step k (timestep
    taus[k - 1]); vs[k - 1] the probe [H, H] of step k, or None for the plain encoder (no q).  With probes the q are
    autograd's and the log-density is accumulated in fp64 with math.log1p (the fp64 definition, not the kernel's
    restated bits).  npos: stop after that many steps.  tables: (ix, ie, g) indexed by the step k to walk with instead of
    :func:`coefficients` (the product's encode_tables, reordered).
    -> dict(x, q [steps, n], acc [n], prior [n], logdet [n], logp [n], invalid [n])."""
    S = len(taus)
    ix, ie, g = coefficients(ab_t, taus, dtype) if tables is None else tables
    x = x0.to(dtype)
    n, D = x.shape[0], x[0].numel()
    acc = torch.zeros(n, dtype=torch.float64)
    qs = []
    for k in range(1, (S if npos is None else npos) + 1):
        if vs is None:
            with torch.no_grad():
                eps = eps_fn(x, k)
        else:
            xin = x.detach().clone().requires_grad_(True)
            eps = eps_fn(xin, k)
            q, _ = vjp_q(eps, xin, vs[k - 1])
            q = q.detach().double()
            gq = float(g[k]) * q
            if form == "trace":
                ld = gq
            else:
                r = gq / D
                ld = torch.where(r > -1, D * torch.log1p(r.clamp_min(-1 + 1e-300)), torch.full_like(r, float("nan")))
            acc = acc + ld
            qs.append(q)
            eps = eps.detach()
        x = (ix[k] * x + ie[k] * eps).detach()
    ab = float(torch.as_tensor(ab_t).double()[taus[-1]])
    prior = -0.5 * x.double().flatten(1).pow(2).sum(1) - 0.5 * D * LOG_2PI
    logdet = 0.5 * D * math.log(ab) + acc
    return dict(x=x, q=torch.stack(qs) if qs else None, acc=acc, prior=prior, logdet=logdet, logp=prior + logdet,
                invalid=torch.isnan(acc))


def oracle_eps(sd, params, guide_w, T, taus, rows, dtype, *, n_feat, n_cfeat, height, kinks=None):
    """eps_fn for :func:`walk` on the oracle's eval forward (oracle/ref_cpu.py) with the CFG combination of the
    samplers: rows[k - 1] = the shortcut draws of step k ([(w, b)] or [(w, b) cond, (w, b) uncond]); kinks(k, half) -> a
    context manager around the forward of half 0 (cond) / 1 (uncond), or None."""
    from oracle import ref_cpu as R
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    c = params.to(dtype) if params is not None else None
    cfg = guide_w > 0 and params is not None
    w = torch.tensor(float(guide_w), dtype=torch.float32).to(dtype)

    def fwd(x, cc, sc, k, half):
        tin = torch.tensor([taus[k - 1] / T]).to(dtype)              # the fp32 value of i / T, as the prologue writes it
        ctx = kinks(k, half) if kinks is not None else None
        if ctx is not None:
            ctx.__enter__()
        try:
            return R.unet_forward(sd, x[:, None], tin, cc, n_feat=n_feat, n_cfeat=n_cfeat, height=height, train=False,
                                  shortcut=(sc[0].to(dtype), sc[1].to(dtype)))[:, 0]
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)

    def eps_fn(x, k):
        ec = fwd(x, c, rows[k - 1][0], k, 0)
        if not cfg:
            return ec
        eu = fwd(x, torch.zeros_like(c), rows[k - 1][1], k, 1)
        return eu + w * (ec - eu)
    return eps_fn


def gaussian_eps(ab_t, taus, s2, dtype=torch.float64):
    """The exact noise prediction of data N(0, s2 I) in the sampler's convention: eps(x, t) = sqrt(1 - ab_t) x /
    (ab_t s2 + 1 - ab_t), so J = c I and v^T J v = c D for every Rademacher v."""
    ab = torch.as_tensor(ab_t).double()

    def eps_fn(x, k):
        a = float(ab[taus[k - 1]])
        return (math.sqrt(1 - a) / (a * s2 + 1 - a)) * x
    return eps_fn


def gaussian_logp(x0, s2):
    """log N(x0; 0, s2 I) per row, fp64."""
    x = x0.double().flatten(1)
    D = x.shape[1]
    return -0.5 * x.pow(2).sum(1) / s2 - 0.5 * D * (LOG_2PI + math.log(s2))
