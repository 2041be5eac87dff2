"""Host side of the parameter fit (cdm_amd.param_fit): argument validation, ScanResult.top, and the restatement the GPU
tests compare against (tests/_fit_ref.py) checked against itself — its gradient by finite differences of its score in
fp64, its update rule on random inputs.  No GPU."""
import numpy as np
import pytest
import torch

import cdm_amd
import _fit_ref as FR
import _parity
import _scan_ref as SR
from cdm_amd import ScanResult, check_fit

NCF, H, T = 6, 64, 20


# ----------------------------------------------------------------------------------------------------------------------
# check_fit
# ----------------------------------------------------------------------------------------------------------------------
def test_check_fit_accepts_the_three_start_shapes():
    maps = np.random.default_rng(0).random((2, 1, H, H))
    for start, K in ((torch.full((NCF,), 0.5), 1), (torch.rand(3, NCF), 3), (torch.rand(2, 4, NCF), 4)):
        x, st, tg, z, mask, lo, hi = check_fit(maps, start, T, NCF, H, n_steps=4)
        assert x.shape == (2, H, H) and x.dtype == torch.float32
        assert st.shape == (2, K, NCF) and st.dtype == torch.float32 and st.is_contiguous()
        assert tg == [5, 10, 15, 20] and z is None
        assert mask.tolist() == [1] * NCF and mask.dtype == torch.int32
        assert lo.tolist() == [0.0] * NCF and hi.tolist() == [1.0] * NCF and lo.dtype == torch.float64
        if start.dim() < 3:
            assert torch.equal(st[0], st[1]) and torch.equal(st[0], start.reshape(-1, NCF))
        else:
            assert torch.equal(st, start)
    _, _, _, _, mask, lo, hi = check_fit(maps, torch.full((NCF,), 0.5), T, NCF, H, n_steps=4, free=[3, 0],
                                         bounds=(np.zeros(NCF), np.arange(1, NCF + 1)))
    assert mask.tolist() == [1, 0, 0, 1, 0, 0] and hi.tolist() == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("kw", [
    dict(start=torch.zeros(NCF - 1)), dict(start=torch.zeros(3, NCF + 1)), dict(start=torch.zeros(3, 2, NCF)),
    dict(start=torch.zeros(1, 2, 2, NCF)), dict(start=torch.zeros(0, NCF)),
    dict(maps=torch.zeros(2, H, H - 1)), dict(maps=torch.zeros(2, 2, H, H)),
    dict(iters=0), dict(iters=2.5), dict(lr=0.0), dict(lr=-1e-3), dict(lr=float("nan")), dict(lr=float("inf")),
    dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(0.9,)),
    dict(free=[NCF]), dict(free=[-1]), dict(free=[0, 2, 0]), dict(free=[]), dict(free=[0.5]),
    dict(bounds=(1.0, 0.0)), dict(bounds=(np.zeros(NCF), np.r_[np.ones(NCF - 1), -1.0])), dict(bounds=(0.0,)),
    dict(bounds=(np.zeros(2), np.ones(2))),
    dict(start=torch.full((NCF,), 1.5)), dict(start=torch.full((NCF,), -0.01)), dict(bounds=(0.3, 0.4)),
    dict(start=torch.full((NCF,), float("nan"))),
    dict(in_channels=2),
    dict(t_grid=[0, 5]), dict(t_grid=[5, 5]), dict(n_noise=0), dict(weight="elbo"), dict(max_rows=1),
    dict(t_grid=[1, 2], noise=torch.zeros(2, 1, H, H)),
])
def test_check_fit_raises_and_touches_nothing(kw):
    """Every listed case is a ValueError from check_fit and from param_fit itself, which raises before it asks the
    model for its engine (the model here lives on the CPU) or draws from the CPU RNG."""
    kw = dict(kw)
    kw.setdefault("n_steps", 4)
    maps, start = kw.pop("maps", torch.zeros(2, H, H)), kw.pop("start", torch.full((NCF,), 0.5))
    in_ch = kw.pop("in_channels", 1)
    with pytest.raises(ValueError):
        check_fit(maps, start, T, NCF, H, in_channels=in_ch, **kw)
    m = cdm_amd.ContextUnet(in_ch, 16, NCF, H)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        cdm_amd.param_fit(m, maps, start, T, **kw)
    assert torch.equal(torch.get_rng_state(), state)
    assert "_cdm_param_fit" not in m.__dict__


def test_scan_result_top_vs_argsort():
    g = np.random.default_rng(3)
    score, cand = g.random((4, 7)), g.random((7, NCF)).astype(np.float32)
    score[2, 3] = score[2, 5]                                   # a tie keeps the candidates' order
    r = ScanResult(torch.from_numpy(score), torch.from_numpy(cand), [1, 10, 20])
    for k in (1, 3, 7):
        top = r.top(k)
        assert top.shape == (4, k, NCF) and top.dtype == torch.float32
        np.testing.assert_array_equal(top.numpy(), cand[np.argsort(score, axis=1, kind="stable")[:, :k]])
    np.testing.assert_array_equal(r.top(1)[:, 0].numpy(), r.best().numpy())
    for k in (0, 8, 1.5, True):
        with pytest.raises(ValueError):
            r.top(k)
    x, st, *_ = check_fit(torch.zeros(4, H, H), r.top(2), T, NCF, H, n_steps=4)      # the natural start
    assert st.shape == (4, 2, NCF)


def test_fit_result_best():
    g = torch.Generator().manual_seed(1)
    params, score = torch.rand(3, 4, NCF, generator=g), torch.rand(3, 4, generator=g).double()
    hist = torch.stack([score + 1, score])
    r = cdm_amd.FitResult(params, score, params, params, hist, hist, torch.zeros(3, 4, dtype=torch.int32), [1, 2])
    assert torch.equal(r.best(), params[torch.arange(3), score.argmin(1)])
    assert torch.equal(r.start_score, hist[0])


# ----------------------------------------------------------------------------------------------------------------------
# the restatement's definition against itself
# ----------------------------------------------------------------------------------------------------------------------
def test_restated_gradient_vs_finite_difference_fp64():
    """n_feat 8, H 64, M = K = 1, P = 2 positions (t = 3 and 17), weight "nll" (so a missing w shows), n_noise 2 of one
    timestep would hide 1/R: t_grid = [10] x n_noise 2 is run as well.  The central difference of score along u = g / |g|
    at h = 1e-3, 1e-4, 1e-5 against |g|: a missing 2, 1/R, w or HW is off by >= 0.3 relative; the bar is 1e-2 at the
    best of the three h (ReLU kinks inside the interval keep this from being a precision claim)."""
    nf = 8
    torch.manual_seed(2)
    m = cdm_amd.ContextUnet(1, nf, NCF, H)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    x = torch.rand(1, H, H, generator=g)
    noise = torch.randn(2, 1, H, H, generator=g)
    c = torch.rand(1, 1, NCF, generator=g).double()
    kw = dict(n_feat=nf, n_cfeat=NCF, height=H)
    for tag, t_grid, R_ in (("two_t", [3, 17], 1), ("two_draws", [10], 2)):
        rows = SR.draw_rows(7, 2, nf)
        ev = lambda cc: FR.evaluate(sd, x, cc, T, t_grid, R_, noise, rows, torch.float64, "nll", **kw)   # noqa: E731
        s0, grad = ev(c)
        gn = grad.norm().item()
        u = grad / gn
        errs = {}
        for h in (1e-3, 1e-4, 1e-5):
            fd = (ev(c + h * u)[0] - ev(c - h * u)[0]).item() / (2 * h)
            errs[h] = abs(fd - gn) / gn
        print(f"[fd/{tag}] score {s0.item():.6e} |g| {gn:.6e} rel err by h: {errs}")
        _parity.record("param_fit_fd", tag=tag, score=s0.item(), gnorm=gn, rel_err={str(h): e for h, e in errs.items()})
        assert min(errs.values()) <= 1e-2, errs


# ----------------------------------------------------------------------------------------------------------------------
# the restated update
# ----------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_restated_update_properties():
    """Random inputs, 3 iterations + the closing pass + one past it: results stay inside the bounds (and reach them),
    non-free columns keep their bits, the best is tracked, a non-finite row stalls with c, m, v unchanged, nothing moves
    once the pass counter is past iters."""
    g = np.random.default_rng(11)
    rows, iters = 9, 3
    free = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    lo, hi = np.full(NCF, 0.2), np.full(NCF, 0.8)
    c0 = g.uniform(0.2, 0.8, (rows, NCF)).astype(np.float32)
    st = FR.new_state(c0, iters)
    bc = FR.bias_table(0.9, 0.999, iters)
    assert bc[0, 0] == 1 - 0.9 and bc[2, 1] == 1 - 0.999 ** 3.0
    args = (iters, free, lo, hi, 0.7, 0.9, 0.999, 1e-8, bc)            # lr 0.7 > hi - lo: the first step leaves [0.2, 0.8]
    scores = g.uniform(1, 2, (iters + 2, rows))
    scores[1, 4], scores[2, 5] = np.nan, np.inf
    seen_best = np.full(rows, np.inf)
    for n in range(iters + 2):
        grad = g.standard_normal((rows, NCF))
        grad[0, 0] = 0.0
        if n == 1:
            grad[6, 2] = np.nan
        before = {k: np.copy(v) for k, v in st.items()}
        FR.update(st, scores[n], grad, *args)
        if n > iters:                                                     # past the closing pass: nothing moves
            assert all(_bits(before[k], st[k]) for k in before)
            continue
        assert st["done"] == n + 1
        assert _bits(st["hist_score"][n], scores[n])
        better = scores[n] < seen_best
        assert _bits(st["best_c"][better], before["c32"][better]) and _bits(st["best_c"][~better], before["best_c"][~better])
        seen_best = np.where(better, scores[n], seen_best)
        assert _bits(st["best_score"], seen_best)
        assert _bits(st["c64"][:, free == 0], c0[:, free == 0].astype(np.float64))
        assert _bits(st["c32"][:, free == 0], c0[:, free == 0])
        assert (st["c64"] >= 0.2).all() and (st["c64"] <= 0.8).all() and _bits(st["c32"], st["c64"].astype(np.float32))
        bad = ~(np.isfinite(scores[n]) & np.isfinite(grad[:, free == 1]).all(1))
        if n < iters:
            assert np.flatnonzero(bad).tolist() == [[], [4, 6], [5]][n]
            for k in ("c64", "c32", "m", "v"):
                assert _bits(st[k][bad], before[k][bad])
            ok = ~bad
            assert (st["c64"][ok][:, free == 1] != before["c64"][ok][:, free == 1]).any()
            assert _bits(st["stalled"], before["stalled"] + bad.astype(np.int32))
        else:                                                             # the closing pass records only
            for k in ("c64", "c32", "m", "v", "stalled"):
                assert _bits(st[k], before[k])
    assert st["stalled"].tolist() == [0, 0, 0, 0, 1, 1, 1, 0, 0]
    # the first Adam step has size lr = 0.7 on every free column with a non-zero gradient: it lands on a bound
    st1 = FR.new_state(c0, iters)
    grad = g.standard_normal((rows, NCF))
    FR.update(st1, scores[0], grad, *args)
    moved = st1["c64"][:, free == 1]
    assert np.isin(moved, (0.2, 0.8)).all()
    assert ((moved == 0.2) == (grad[:, free == 1] > 0)).all()
    # a gradient of exactly 0 leaves m = v = 0 and c unchanged: 0 / (sqrt(0) + eps) = 0
    st0 = FR.new_state(c0, iters)
    FR.update(st0, scores[0], np.zeros((rows, NCF)), *args)
    assert _bits(st0["c64"], c0.astype(np.float64)) and not st0["m"].any() and not st0["v"].any()
