"""Host side of the strided (DDIM) sampler: timestep subsequences and the coefficient tables (no GPU, no library).

The update (cdm_amd.diffusion.ddim_tables), from i = tau_k to j = tau_{k-1} (tau_0 = 0, ab_0 = 1):
    sigma = eta sqrt((1 - ab_j) / (1 - ab_i)) sqrt(1 - ab_i / ab_j)
    cx = sqrt(ab_j / ab_i);  ce = sqrt(1 - ab_j - sigma^2) - sqrt(ab_j (1 - ab_i) / ab_i)
"""
import numpy as np
import pytest
import torch

import _parity
from oracle import ref_cpu as R


def _fns():
    from cdm_amd.diffusion import ddim_tables, timestep_subsequence
    return timestep_subsequence, ddim_tables


def test_subsequences():
    ts, _ = _fns()
    assert ts(1500, 50, "uniform") == list(range(30, 1501, 30))
    assert ts(1500, 50) == ts(1500, 50, "uniform")
    q = ts(100, 50, "quadratic")
    assert len(q) == 50 and q[0] == 1 and q[-1] == 100
    assert all(b > a for a, b in zip(q, q[1:]))
    assert q == [max(-(-k * k // 25), k) for k in range(1, 51)]          # ceil(100 (k / 50)^2) = ceil(k^2 / 25)
    for T in (1, 7, 100):
        for sp in ("uniform", "quadratic"):
            assert ts(T, T, sp) == list(range(1, T + 1))
    assert ts(100, 7) == [14, 29, 43, 57, 71, 86, 100]          # round(k 100 / 7)
    assert ts(100, None, [3, 50, 100]) == [3, 50, 100]
    assert ts(100, 3, (3, 50, 100)) == [3, 50, 100]
    assert ts(100, None, torch.tensor([1, 100])) == [1, 100]
    for T, S in ((1500, 50), (1500, 7), (100, 12), (100, 13), (20, 5), (11, 10)):
        for sp in ("uniform", "quadratic"):
            tau = ts(T, S, sp)
            assert len(tau) == S and tau[0] >= 1 and tau[-1] == T and all(b > a for a, b in zip(tau, tau[1:]))


@pytest.mark.parametrize("S,spacing", [
    (None, [10, 10, 100]),       # not increasing
    (None, [50, 10, 100]),       # decreasing
    (None, [10, 50, 99]),        # last entry is not T
    (None, [10, 50, 101]),
    (None, [0, 50, 100]),        # first entry below 1
    (None, [-3, 100]),
    (None, []),
    (2, [10, 50, 100]),          # S disagrees with the list
    (None, [10.5, 100]),         # not integers
    (101, "uniform"),            # S > T
    (101, "quadratic"),
    (0, "uniform"),
    (None, "uniform"),
    (10, "cosine"),
])
def test_bad_subsequences_raise(S, spacing):
    ts, _ = _fns()
    with pytest.raises(ValueError):
        ts(100, S, spacing)


def _identity_errors(b_t, a_t, ab_t):
    """max relative deviation over k = 2..T of the eta = 1 full-sequence tables from the ancestral coefficients, in fp64
    on the fp32 schedule tables: against the a_t / b_t tables, and against a'_k = ab_k / ab_{k-1} (b' = 1 - a')."""
    ts, tables = _fns()
    T = ab_t.numel() - 1
    cx, ce, sg = (v.astype(np.float64) for v in tables(ab_t, ts(T, T), 1.0))
    a, ab, b = (v.double().numpy() for v in (a_t, ab_t, b_t))
    k = np.arange(2, T + 1)
    out = {}
    for name, ak, bk in (("table", a[k], b[k]), ("ratio", ab[k] / ab[k - 1], 1 - ab[k] / ab[k - 1])):
        out[name] = (float(np.abs(cx[k] * np.sqrt(ak) - 1).max()),
                     float(np.abs(ce[k] / (-(1 - ak) / (np.sqrt(1 - ab[k]) * np.sqrt(ak))) - 1).max()),
                     float(np.abs(sg[k] ** 2 / (bk * (1 - ab[k - 1]) / (1 - ab[k])) - 1).max()))
    return out


# observed maxima (cx, ce, sigma^2) of _identity_errors(...)["table"] on the committed schedules, see the docstring below
OBSERVED = {400: (1.59e-7, 1.01e-4, 1.07e-4), 1500: (4.94e-7, 3.40e-4, 4.15e-4)}


@pytest.mark.parametrize("T", [400, 1500])
def test_full_sequence_eta1_is_the_ancestral_mean(T):
    """Over 1..T with eta = 1 the update is denoise_add_noise's mean and the posterior variance, for every k >= 2:
        cx[k] == 1 / sqrt(a_k),  ce[k] == -(1 - a_k) / (sqrt(1 - ab_k) sqrt(a_k)),
        sigma[k]^2 == b_k (1 - ab_{k-1}) / (1 - ab_k),
    compared in fp64 on the committed fp32 schedules (tests/golden/schedule.npz: fixed inputs, so the figures below are
    the same on every host).

    The tables are built from ab alone, and ab (exp of an fp32 cumulative sum of logs) is only fp32-consistent with the
    a_t table: ab_k / ab_{k-1} differs from a_k by d ~ 1e-7 .. 1e-6 relative.  cx sees d / 2.  ce and sigma^2 are
    proportional to 1 - a_k = b_k, which is 1e-4 .. 2e-2, so they see d / b_k, up to ~1e-7 / 1e-4 = 1e-3 relative at the
    small-k end — not the 1e-6 the identity would hold to on a consistent schedule.  Two comparisons, therefore:
      * against a'_k = ab_k / ab_{k-1} (and b'_k = 1 - a'_k), the step the tables actually encode: what is left is the
        one fp32 rounding of each table entry, 2^-24 = 6.0e-8 relative (1.2e-7 for sigma^2); bar 1e-6.
        Observed: T = 400: cx 5.9e-8, ce 5.8e-8, sigma^2 1.2e-7; T = 1500: cx 5.9e-8, ce 5.9e-8, sigma^2 1.2e-7.
      * against the a_t / b_t tables themselves; bar 4x the observed maximum (OBSERVED above):
        T = 400: cx 1.59e-7, ce 1.01e-4, sigma^2 1.07e-4; T = 1500: cx 4.94e-7, ce 3.40e-4, sigma^2 4.15e-4."""
    b_t, a_t, ab_t = _parity.golden_schedule(T)
    err = _identity_errors(b_t, a_t, ab_t)
    print(f"T={T}: vs a_t table cx/ce/sigma^2 {err['table']}, vs ab ratio {err['ratio']}")
    for e in err["ratio"]:
        assert e <= 1e-6, err
    for e, obs in zip(err["table"], OBSERVED[T]):
        assert e <= 4 * obs, err


def test_full_sequence_identity_on_this_host_schedule():
    """The same identity on the schedule built on this host (T = 100), against the ab ratio: 1e-6 (see above)."""
    err = _identity_errors(*R.make_schedule(100))
    for e in err["ratio"]:
        assert e <= 1e-6, err


@pytest.mark.parametrize("spacing", ["uniform", "quadratic"])
def test_eta0_has_no_noise(spacing):
    ts, tables = _fns()
    _, _, ab_t = R.make_schedule(100)
    cx, ce, sg = tables(ab_t, ts(100, 12, spacing), 0.0)
    assert cx.dtype == ce.dtype == sg.dtype == np.float32 and cx.shape == ce.shape == sg.shape == (13,)
    assert (sg == 0).all()
    assert (cx[1:] > 1).all() and (ce[1:] < 0).all()
    assert (cx[0], ce[0], sg[0]) == (1.0, 0.0, 0.0)              # the unused entry 0


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_last_position(eta):
    """The step to tau_0 = 0 (ab_0 = 1): x_0 = (x_i - sqrt(1 - ab_i) eps) / sqrt(ab_i), no noise, whatever eta is."""
    ts, tables = _fns()
    _, _, ab_t = R.make_schedule(100)
    for tau in (ts(100, 7), ts(100, 100), [5, 100]):
        cx, ce, sg = tables(ab_t, tau, eta)
        abi = float(ab_t[tau[0]].double())
        assert sg[1] == 0
        assert cx[1] == np.float32(1 / np.sqrt(abi))
        assert ce[1] == np.float32(-np.sqrt((1 - abi) / abi))
        if eta > 0 and len(tau) > 1:
            assert (sg[2:] > 0).all()


def test_tables_follow_the_definition():
    """Every entry against the formulas, term by term in fp64 (python floats), rounded once to fp32."""
    import math
    ts, tables = _fns()
    _, _, ab_t = R.make_schedule(100)
    tau = ts(100, 7)
    ab = [float(v) for v in ab_t.double()]
    for eta in (0.0, 0.5, 1.0):
        cx, ce, sg = tables(ab_t, tau, eta)
        for k in range(1, 8):
            i, j = tau[k - 1], (tau[k - 2] if k > 1 else 0)
            s = eta * math.sqrt((1 - ab[j]) / (1 - ab[i])) * math.sqrt(1 - ab[i] / ab[j]) if j else 0.0
            assert sg[k] == np.float32(s)
            assert cx[k] == np.float32(math.sqrt(ab[j] / ab[i]))
            assert ce[k] == np.float32(math.sqrt(1 - ab[j] - s * s) - math.sqrt(ab[j] * (1 - ab[i]) / ab[i]))


def test_tables_reject_bad_input():
    _, tables = _fns()
    _, _, ab_t = R.make_schedule(100)
    with pytest.raises(ValueError):
        tables(ab_t, [10, 50, 99], 0.0)          # does not end at T
    with pytest.raises(ValueError):
        tables(ab_t, [10, 100], -0.1)
    with pytest.raises(ValueError):
        tables(ab_t, [10, 100], 50.0)            # sigma^2 > 1 - ab_j
