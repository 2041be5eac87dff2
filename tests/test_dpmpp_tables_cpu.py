"""Host side of the multistep (DPM-Solver++ 2M) sampler: the coefficient tables and the order of accuracy they give
(no GPU, no library).

The update (cdm_amd.diffusion.dpmpp_tables, restated in tests/_dpmpp_ref.py), from i = tau_k to j = tau_{k-1}
(tau_0 = 0, ab_0 = 1, alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma), h_k = lambda_j - lambda_i):
    sq = sigma_i, ra = 1 / alpha_i, cx = sigma_j / sigma_i, cd = alpha_j - sigma_j alpha_i / sigma_i
    order 2, 1 < k < S: r = h_{k+1} / h_k, c0 = 1 + 1 / (2 r), c1 = -1 / (2 r);  otherwise c0 = 1, c1 = 0
    d = (x - sq eps) ra;  D = d if c1 == 0 else c0 d + c1 d_prev;  x_j = cx x + cd D
"""
import math

import numpy as np
import pytest
import torch

import _dpmpp_ref as P
from oracle import ref_cpu as R

NAMES = ("sq", "ra", "c0", "c1", "cx", "cd")


def _fns():
    from cdm_amd.diffusion import ddim_tables, dpmpp_tables, timestep_subsequence
    return timestep_subsequence, dpmpp_tables, ddim_tables


def _schedule(T):
    """The project's default schedule (fp32 expressions of diffusion.Schedule), ab_t as an fp32 CPU tensor."""
    return R.make_schedule(T)[2]


@pytest.mark.parametrize("order", [1, 2])
def test_tables_are_the_fp64_definition_rounded_once(order):
    """Every entry against the restatement's python-float formulas: the fp64 tables to 1e-13 relative, the fp32 tables
    equal to those fp64 values rounded once.  (1e-13: numpy's and libm's log may differ in the last bit, 2^-52 |lambda|
    with |lambda| < 9 on this schedule, i.e. 2e-15; h is a difference of two, >= 0.1 for these sequences, and c0 - 1 and
    c1 a ratio of two h: 4 x 2e-15 / 0.1 = 8e-14.  Everything else is the same IEEE sqrt / divide on both sides.)"""
    ts, tables, _ = _fns()
    ab_t = _schedule(1500)
    for tau in (ts(1500, 20), ts(1500, 20, "quadratic"), [2, 50, 100, 1500], [1500], [7, 1500]):
        ref = [v.numpy() for v in P.coefficients(ab_t, tau, order, torch.float64)]
        t64 = tables(ab_t, tau, order, dtype=np.float64)
        t32 = tables(ab_t, tau, order)
        for name, r, a, b in zip(NAMES, ref, t64, t32):
            assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape == (len(tau) + 1,), name
            assert np.all(np.abs(a - r) <= 1e-13 * np.abs(r)), name
            assert np.array_equal(b, a.astype(np.float32)), name


def test_order1_is_ddim_eta0():
    """order = 1, uniform S = 20 of T = 1500, in fp64: x_j = cx x + cd (x - sq eps) ra = (cx + cd ra) x - cd ra sq eps,
    so cx + cd ra and -cd ra sq are DDIM's cx and ce at eta = 0 (recomputed here in fp64 from the formulas of
    ddim_tables, whose fp32 output must be these values rounded).  Bar 1e-12 relative (observed 2.8e-16 and 6.3e-16)."""
    ts, tables, ddim_tables = _fns()
    ab_t = _schedule(1500)
    tau = ts(1500, 20)
    sq, ra, c0, c1, cx, cd = (v[1:] for v in tables(ab_t, tau, 1, dtype=np.float64))
    assert (c0 == 1).all() and (c1 == 0).all()
    ab = ab_t.double().numpy()
    ab_i = ab[np.array(tau)]
    ab_j = np.concatenate([[1.0], ab[np.array(tau[:-1])]])
    dcx = np.sqrt(ab_j / ab_i)
    dce = np.sqrt(1 - ab_j) - np.sqrt(ab_j * (1 - ab_i) / ab_i)
    d32 = ddim_tables(ab_t, tau, 0.0)
    assert np.array_equal(d32[0][1:], dcx.astype(np.float32)) and np.array_equal(d32[1][1:], dce.astype(np.float32))
    e_cx = float(np.abs((cx + cd * ra) / dcx - 1).max())
    e_ce = float(np.abs((-cd * ra * sq) / dce - 1).max())
    print(f"order 1 vs DDIM eta = 0: cx {e_cx:.2e}, ce {e_ce:.2e}")
    assert e_cx <= 1e-12 and e_ce <= 1e-12


def test_structure():
    ts, tables, _ = _fns()
    ab_t = _schedule(100)
    for tau in (ts(100, 12), ts(100, 13, "quadratic"), ts(100, 100), [2, 50, 100]):
        S = len(tau)
        sq, ra, c0, c1, cx, cd = tables(ab_t, tau, 2)
        assert all(v.dtype == np.float32 and v.shape == (S + 1,) for v in (sq, ra, c0, c1, cx, cd))
        assert (sq[0], ra[0], c0[0], c1[0], cx[0], cd[0]) == (0.0, 1.0, 1.0, 0.0, 1.0, 0.0)      # the unused entry 0
        assert c1[S] == 0 and c1[1] == 0 and c0[S] == 1 and c0[1] == 1
        assert cx[1] == 0 and cd[1] == 1
        assert (c1[2:S] < 0).all() and (c0[2:S] > 1).all()
        assert (np.abs((c0.astype(np.float64) + c1.astype(np.float64)) - 1) <= np.spacing(np.float32(1))).all()
        assert (cx[2:] > 0).all() and (cx[1:] < 1).all() and (cd[1:] > 0).all()
        o1 = tables(ab_t, tau, 1)
        assert (o1[2] == 1).all() and (o1[3] == 0).all()
        for a, b in zip((sq, ra, cx, cd), (o1[0], o1[1], o1[4], o1[5])):
            assert np.array_equal(a, b)                                   # the order only changes c0 / c1
    for tau in ([100], [40, 100]):                                        # S <= 2: first order throughout
        for a, b in zip(tables(ab_t, tau, 2), tables(ab_t, tau, 1)):
            assert np.array_equal(a, b)
    assert tables(ab_t, [2, 50, 100], 2)[0].shape == (4,)
    assert tables(ab_t, torch.tensor([2, 50, 100]), 2)[3][2] != 0


def test_bad_input_raises():
    ts, tables, _ = _fns()
    ab_t = _schedule(100)
    for order in (3, 0, 1.5, "2", True):
        with pytest.raises(ValueError):
            tables(ab_t, ts(100, 12), order)
    with pytest.raises(ValueError):
        tables(ab_t, [10, 50, 99], 2)                # does not end at T
    for bad in (torch.ones(101), torch.zeros(101), torch.linspace(0.1, 0.9, 101)):    # sigma = 0; alpha = 0; ab growing
        bad = bad.clone(); bad[0] = 1
        with pytest.raises(ValueError):
            tables(bad, ts(100, 12), 2)
    nan = ab_t.clone(); nan[50] = float("nan")
    with pytest.raises(ValueError):
        tables(nan, [50, 100], 2)


# ---------------------------------------------------------------------------------------------------------------
# order of accuracy on a Gaussian data distribution
# ---------------------------------------------------------------------------------------------------------------
T_, MU, SD = 1500, 0.4, 0.25


def _gaussian_errors():
    """RMS error of the sampled x_0 against the exact solution of the sampling ODE, per (order, S), in fp64.

    Data x_0 ~ N(mu, s^2): x_i ~ N(alpha_i mu, ab_i s^2 + 1 - ab_i), so the exact noise prediction is
    eps(x, i) = sigma_i (x - alpha_i mu) / (ab_i s^2 + 1 - ab_i), and the ODE transports quantiles:
    x_0 = mu + s (x_T - alpha_T mu) / sqrt(ab_T s^2 + 1 - ab_T)."""
    ts, tables, _ = _fns()
    ab_t = _schedule(T_)
    ab = ab_t.double()
    x_T = torch.from_numpy(np.random.default_rng(0).standard_normal(64))

    def eps(x, t, c):
        i = int(round(float(t) * T_))
        return torch.sqrt(1 - ab[i]) * (x - torch.sqrt(ab[i]) * MU) / (ab[i] * SD ** 2 + 1 - ab[i])
    exact = MU + SD * (x_T - torch.sqrt(ab[T_]) * MU) / torch.sqrt(ab[T_] * SD ** 2 + 1 - ab[T_])
    err = {}
    for order in (1, 2):
        for S in (80, 160):
            tau = ts(T_, S)
            x, _ = P.sample_loop(eps, x_T, None, 0.0, T_, tau, tables(ab_t, tau, order, dtype=np.float64))
            assert x.dtype == torch.float64
            err[order, S] = float((x - exact).pow(2).mean().sqrt())
    return err


def test_order_of_accuracy():
    """T = 1500 uniform, mu = 0.4, s = 0.25, 64 draws of default_rng(0), tests/_dpmpp_ref.sample_loop in fp64 on fp64
    tables.  Order 2's error at S = 160 is <= 1/4 of order 1's (computed: 0.11); the observed order
    log2(err(80) / err(160)) is >= 1.7 for order 2 (computed: 2.20) and within [0.7, 1.3] for order 1 (computed: 0.95)."""
    err = _gaussian_errors()
    p1 = math.log2(err[1, 80] / err[1, 160])
    p2 = math.log2(err[2, 80] / err[2, 160])
    print(f"rms error vs the exact ODE solution: {err}; observed order {p1:.3f} (order 1), {p2:.3f} (order 2); "
          f"ratio at S = 160: {err[2, 160] / err[1, 160]:.3f}")
    assert err[2, 160] <= err[1, 160] / 4
    assert p2 >= 1.7
    assert 0.7 <= p1 <= 1.3
