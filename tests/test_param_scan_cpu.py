"""Host side of the parameter scan (cdm_amd.param_scan): the candidate grid, the ScanResult methods against numpy on a
hand-made score matrix, and the argument validation, which runs before anything touches a device.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

import cdm_amd
from cdm_amd import ScanResult, check_scan, param_grid

H, NCF, T = 64, 6, 20


def test_param_grid_shape_and_order():
    base = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    g = param_grid(base, {4: (0.0, 1.0, 3), 1: (-1.0, 1.0, 2)})
    assert g.shape == (6, 6) and g.dtype == torch.float32
    want = []
    for a, b in itertools.product(np.linspace(0.0, 1.0, 3), np.linspace(-1.0, 1.0, 2)):   # last axis fastest
        row = np.array(base)
        row[4], row[1] = a, b
        want.append(row)
    np.testing.assert_array_equal(g.numpy(), np.array(want).astype(np.float32))
    # no axes: the base alone; one value per axis: lo
    assert torch.equal(param_grid(base, {}), torch.tensor([base]))
    assert torch.equal(param_grid(torch.tensor(base), {0: (2.0, 5.0, 1)})[0], torch.tensor([2.0] + base[1:]))
    for bad in ({6: (0, 1, 2)}, {-1: (0, 1, 2)}, {0: (0, 1, 0)}, {0: (0, 1)}, {0.5: (0, 1, 2)}):
        with pytest.raises(ValueError):
            param_grid(base, bad)


def test_scan_result_against_numpy():
    score = np.array([[3.0, 1.0, 2.0, 1.5], [0.25, 0.75, 0.5, 4.0]])
    cand = np.array([[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [2.0, -1.0]], dtype=np.float32)
    r = ScanResult(torch.from_numpy(score), torch.from_numpy(cand), [1, 10, 20], n_noise=2, weight="nll")
    assert r.t_grid == [1, 10, 20] and r.n_noise == 2 and r.weight == "nll"
    scale = 2.5
    lw = -scale * (score - score.min(1, keepdims=True))
    np.testing.assert_allclose(r.log_weights(scale).numpy(), lw, rtol=0, atol=1e-15)
    assert (r.log_weights(scale).max(1).values == 0).all()
    w = np.exp(lw) / np.exp(lw).sum(1, keepdims=True)
    mean = w @ cand.astype(np.float64)
    std = np.sqrt((w[:, :, None] * (cand[None].astype(np.float64) - mean[:, None]) ** 2).sum(1))
    gm, gs, gw = r.posterior(scale)
    assert gm.shape == (2, 2) and gs.shape == (2, 2) and gw.shape == (2, 4) and gw.dtype == torch.float64
    np.testing.assert_allclose(gw.numpy(), w, rtol=1e-14)
    np.testing.assert_allclose(gm.numpy(), mean, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(gs.numpy(), std, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(gw.sum(1).numpy(), 1.0, rtol=1e-15)
    assert r.best_index().tolist() == [1, 0]
    np.testing.assert_array_equal(r.best().numpy(), cand[[1, 0]])
    # a large scale concentrates on the best candidate, scale 0 weighs all alike
    np.testing.assert_allclose(r.posterior(1e6)[0].numpy(), cand[[1, 0]], atol=1e-12)
    np.testing.assert_allclose(r.posterior(0.0)[2].numpy(), 0.25)
    with pytest.raises(TypeError):
        r.posterior()                                   # scale has no default


def test_check_scan_normalises():
    maps = np.random.default_rng(0).random((2, 1, H, H))
    x, c, tg, z = check_scan(maps, np.zeros((3, NCF)), T, NCF, H, n_steps=4)
    assert x.shape == (2, H, H) and x.dtype == torch.float32 and c.shape == (3, NCF) and c.dtype == torch.float32
    assert tg == cdm_amd.timestep_subsequence(T, 4) == [5, 10, 15, 20] and z is None
    x, c, tg, z = check_scan(torch.zeros(2, H, H), torch.zeros(1, NCF), T, NCF, H, t_grid=[1, 10, T], n_noise=2,
                             noise=np.zeros((6, 2, H, H)))
    assert tg == [1, 10, T] and z.shape == (6, 2, H, H) and z.dtype == torch.float32


@pytest.mark.parametrize("kw", [
    dict(t_grid=[0, 5]), dict(t_grid=[5, T + 1]), dict(t_grid=[5, 5]), dict(t_grid=[]), dict(t_grid=[1.5]),
    dict(n_steps=T + 1), dict(max_rows=1), dict(cand=torch.zeros(3, NCF - 1)), dict(cand=torch.zeros(NCF)),
    dict(t_grid=[1, 2], noise=torch.zeros(2, 2, H, H), n_noise=2), dict(t_grid=[1, 2], noise=torch.zeros(2, 1, H, H)),
    dict(t_grid=[1, 2], noise=torch.zeros(2, 2, 1, H, H)), dict(n_noise=0), dict(weight="elbo"),
    dict(maps=torch.zeros(2, H, H - 1)), dict(maps=torch.zeros(2, 2, H, H)),
])
def test_argument_validation(kw):
    """t_grid outside 1..T (or not increasing), M > max_rows, a candidate width other than n_cfeat, a noise table that
    is not [P, M, H, H], and the rest of check_scan's rules: ValueError from the host check and from param_scan itself,
    which raises before it asks the model for its engine (the model here lives on the CPU) or draws from the CPU RNG."""
    kw = dict(kw)
    maps, cand = kw.pop("maps", torch.zeros(2, H, H)), kw.pop("cand", torch.zeros(3, NCF))
    with pytest.raises(ValueError):
        check_scan(maps, cand, T, NCF, H, **kw)
    m = cdm_amd.ContextUnet(1, 16, NCF, H)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        cdm_amd.param_scan(m, maps, cand, T, **kw)
    assert torch.equal(torch.get_rng_state(), state)
    assert "_cdm_param_scan" not in m.__dict__
