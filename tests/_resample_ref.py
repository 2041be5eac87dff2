"""Restatement of position programs (RePaint resampling, late start) on the CPU, independent of cdm_amd: the definition
the GPU tests pin them to.

The program.  taus ascending, tau_0 = 0; a late start keeps the taus <= t_start (S' of them).  State indices k that are
multiples of J with J <= k <= S' - J are jump points, each good for R - 1 jumps.  From k = S', while k > 0: emit the
position (i, j, u) = (tau_k, tau_{k-1}, tau_{k-1}); k -= 1; if k is a jump point with jumps left, use one: the position
just emitted gets u = tau_{k+J}, and k += J.  Positions are numbered P..1 in the order they run.

One position: the solver's step from i to j (tests/_ddim_ref.step or tests/_dpmpp_ref.step, unchanged), the blend at the
level j (tests/_inpaint_ref.blend, unchanged), the snapshot, then, where u != j, the forward jump of the whole state
    x_u = fa x_j + fb zeta,     fa = sqrt(ab_u / ab_j),  fb = sqrt(1 - ab_u / ab_j),  zeta standard normal
two products and a sum, one rounding each.  DPM-Solver++ forgets d_prev after a jump: the next position is first order.

CPU-RNG order: the "fixed" xi once before the loop; per position z (where the solver draws one), the "fresh" xi (where
j >= 1), zeta (where the position jumps), then the shortcut draw(s) inside ``model`` (cond first, then uncond).

Coefficients are evaluated in fp64 (python floats) from the fp32 ab_t table and, for an fp32 run, rounded once to fp32.
"""
import math

import torch

import _ddim_ref as D
import _dpmpp_ref as P
import _inpaint_ref as I


def program(taus, jump=1, resamples=1, t_start=None):
    """[(i, j, u)] in the order the positions run (the first is position P, the last position 1)."""
    tau = [0] + [t for t in taus if t_start is None or t <= t_start]
    S = len(tau) - 1
    left = {k: resamples - 1 for k in range(jump, S - jump + 1, jump)}
    out = []
    k = S
    while k > 0:
        out.append((tau[k], tau[k - 1], tau[k - 1]))
        k -= 1
        if left.get(k, 0) > 0:
            left[k] -= 1
            out[-1] = (out[-1][0], out[-1][1], tau[k + jump])
            k += jump
    return out


def _ab(ab_t):
    ab = [float(v) for v in ab_t.double()]
    ab[0] = 1.0
    return ab


def _t(v, dtype):
    return torch.tensor(v, dtype=torch.float64).to(dtype)


def jump_coefficients(ab_t, prog, dtype=torch.float32):
    """(fa, fb) by run order; (1, 0) exactly where the position does not jump."""
    ab = _ab(ab_t)
    fa = [math.sqrt(ab[u] / ab[j]) if u != j else 1.0 for _, j, u in prog]
    fb = [math.sqrt(1 - ab[u] / ab[j]) if u != j else 0.0 for _, j, u in prog]
    return _t(fa, dtype), _t(fb, dtype)


def ddim_coefficients(ab_t, prog, eta, dtype=torch.float32):
    """(cx, ce, sigma) by run order: tests/_ddim_ref.coefficients' expressions on the pair (i, j) of each position."""
    ab = _ab(ab_t)
    cx, ce, sg = [], [], []
    for i, j, _ in prog:
        s = eta * math.sqrt((1 - ab[j]) / (1 - ab[i])) * math.sqrt(1 - ab[i] / ab[j]) if j else 0.0
        sg.append(s)
        cx.append(math.sqrt(ab[j] / ab[i]))
        ce.append(math.sqrt(1 - ab[j] - s * s) - math.sqrt(ab[j] * (1 - ab[i]) / ab[i]))
    return tuple(_t(v, dtype) for v in (cx, ce, sg))


def dpmpp_coefficients(ab_t, prog, order=2, dtype=torch.float32):
    """(sq, ra, c0, c1, cx, cd) by run order: tests/_dpmpp_ref.coefficients' expressions on the pair of each position.
    Second order only where a previous position exists, it did not jump, and this one does not land on 0; r is the
    previous position's h over this one's."""
    ab = _ab(ab_t)
    lam = lambda t: math.inf if t == 0 else math.log(math.sqrt(ab[t]) / math.sqrt(1 - ab[t]))    # noqa: E731
    h = [lam(j) - lam(i) for i, j, _ in prog]
    sq, ra, c0, c1, cx, cd = [], [], [], [], [], []
    for q, (i, j, _) in enumerate(prog):
        al_i, al_j, sg_i, sg_j = math.sqrt(ab[i]), math.sqrt(ab[j]), math.sqrt(1 - ab[i]), math.sqrt(1 - ab[j])
        sq.append(sg_i)
        ra.append(1 / al_i)
        cx.append(sg_j / sg_i)
        cd.append(al_j - sg_j * al_i / sg_i)
        if order == 2 and q > 0 and prog[q - 1][2] == prog[q - 1][1] and j != 0:
            r = h[q - 1] / h[q]
            c0.append(1 + 1 / (2 * r))
            c1.append(-1 / (2 * r))
        else:
            c0.append(1.0)
            c1.append(0.0)
    return tuple(_t(v, dtype) for v in (sq, ra, c0, c1, cx, cd))


def forward_jump(x, fa, fb, zeta):
    """x_u = fa x_j + fb zeta in separate tensor ops (one rounding each)."""
    a = fa * x
    b = fb * zeta
    return a + b


def _draw(x):
    return torch.randn(x.shape).to(x.dtype)          # an fp32 draw, cast: the fp64 run sees the identical numbers


class _NoBlend:
    def draw(self, x, j):
        pass

    def __call__(self, x, j):
        return x


def _loop(kind, model, x, params, guide_w, T, ab_t, prog, opt, known, mask, mode, save_rate):
    dt = x.dtype
    n = len(prog)
    if kind == "ddim":
        eta = opt
        coef = ddim_coefficients(ab_t, prog, eta, dt)
    else:
        coef = dpmpp_coefficients(ab_t, prog, opt, dt)
    fa, fb = jump_coefficients(ab_t, prog, dt)
    bl = I._Blender(x, ab_t, known, mask, mode) if known is not None else _NoBlend()     # "fixed" xi: before the loop
    cfg = guide_w > 0 and params is not None
    uncond = torch.zeros_like(params) if params is not None else None
    w = torch.tensor(guide_w, dtype=dt)
    d_prev = None
    inter = []
    for q, (i, j, u) in enumerate(prog):
        p = n - q
        t = torch.tensor([i / T]).to(dt)
        z = _draw(x) if kind == "ddim" and eta > 0 and j >= 1 else None
        bl.draw(x, j)
        zeta = _draw(x) if u != j else None
        if cfg:
            ec = model(x, t, params)
            eu = model(x, t, uncond)
        else:
            ec, eu = model(x, t, params), None
        if kind == "ddim":
            x = D.step(x, ec, eu, w, coef[0][q], coef[1][q], coef[2][q], z)
        else:
            x, d_prev = P.step(x, ec, eu, w, *(c[q] for c in coef), d_prev)
        x = bl(x, j)
        if D.snap(p, n, save_rate):
            inter.append(x.clone())
        if u != j:
            x = forward_jump(x, fa[q], fb[q], zeta)
    return x, torch.stack(inter)


def ddim_loop(model, x, params, guide_w, T, ab_t, prog, eta, known=None, mask=None, mode="fixed", save_rate=20):
    """tests/_inpaint_ref.ddim_loop over a program (``known`` None: no blend); x is the state at the level of the first
    position.  Snapshots hold the blended state before the jump."""
    return _loop("ddim", model, x, params, guide_w, T, ab_t, prog, eta, known, mask, mode, save_rate)


def dpmpp_loop(model, x, params, guide_w, T, ab_t, prog, order, known=None, mask=None, mode="fixed", save_rate=20):
    """tests/_inpaint_ref.dpmpp_loop over a program; c1 = 0 after a jump, so the stale d_prev is never read."""
    return _loop("dpmpp", model, x, params, guide_w, T, ab_t, prog, order, known, mask, mode, save_rate)
