"""Torch-CPU restatement of the parameter scan's definition (likelihood.ParamScan) on the oracle's forward.

Positions p = r S + s (timestep t_grid[s], repeat r of R), one noise map z_p[m] and one shortcut row per position, both
common to every candidate:
    x_p[m]     = sab[t_p] x[m] + omab[t_p] z_p[m]          in fp32, perturb_input's roundings (an input of the network,
                                                           the same fp32 values in the fp32 and the fp64 run)
    eps_p[m,k] = unet_forward(eval)(x_p[m], t_p / T, c[k])  in ``dtype``; t_p / T is the fp32 value the reference passes
    mse[p,m,k] = mean_pixels (eps_p[m,k] - z_p[m])^2        the difference in ``dtype``, squares and sum in fp64
    score[m,k] = (1 / R) sum_p w[t_p] mse[p,m,k]            fp64; w = 1 or the fp32 rounding of 1 / (2 b_t)
Every candidate is run in a forward of its own at batch M, so a candidate's result does not depend on which others are
scanned with it.  The shortcut rows are drawn here, after reseeding the CPU RNG, one per position p = 0..P-1 in order:
the draws param_scan makes after the same torch.manual_seed."""
import torch

from oracle import ref_cpu as R


def draw_rows(seed: int, P: int, n_feat: int):
    torch.manual_seed(seed)
    return [R.draw_shortcut(1, n_feat) for _ in range(P)]


def weights(kind: str, T: int) -> torch.Tensor:
    """w [T + 1] fp64: the values of the fp32 table the scan reads."""
    b_t, _, _ = R.make_schedule(T)
    if kind == "uniform":
        return torch.ones(T + 1, dtype=torch.float64)
    assert kind == "nll"
    return (1.0 / (2.0 * b_t.double())).float().double()


def position_mse(sd, x, cand, T, t_grid, n_noise, noise, rows, dtype, *, n_feat, n_cfeat, height):
    """mse [P, M, K] fp64 of the definition with the network run in ``dtype``.  x [M,H,H], cand [K,ncf], noise [P,M,H,H]
    fp32; rows = draw_rows(...)."""
    _, _, ab_t = R.make_schedule(T)
    sab, omab = ab_t.sqrt(), 1 - ab_t
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    M, K, S = x.shape[0], cand.shape[0], len(t_grid)
    P = S * n_noise
    assert noise.shape == (P, M, height, height) and len(rows) == P
    out = torch.zeros(P, M, K, dtype=torch.float64)
    with torch.no_grad():
        for p in range(P):
            t = t_grid[p % S]
            z = noise[p]
            xp = sab[t] * x + omab[t] * z                                   # fp32, two products and a sum
            tin = torch.tensor([t / T])                                      # fp32 rounding of the fp64 quotient
            w, b = rows[p]
            for k in range(K):
                eps = R.unet_forward(sd, xp[:, None].to(dtype), tin.to(dtype), cand[k].expand(M, -1).to(dtype),
                                     n_feat=n_feat, n_cfeat=n_cfeat, height=height, train=False,
                                     shortcut=(w.to(dtype), b.to(dtype)))
                d = (eps[:, 0] - z.to(dtype)).double()
                out[p, :, k] = (d * d).sum((1, 2)) / (height * height)
    return out


def score(mse, T, t_grid, n_noise, kind):
    """score [M, K] fp64 from position_mse's output."""
    w = weights(kind, T)
    S = len(t_grid)
    wp = torch.stack([w[t_grid[p % S]] for p in range(mse.shape[0])])
    return (wp[:, None, None] * mse).sum(0) / n_noise
