"""Observation-guided sampling, the parts that need no GPU: the restatement's own correctness (tests/_guided_ref.py:
adjoint identity, its gradient against fp64 autograd and a finite difference), the host tables, the argument checks."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _ddim_ref as D
import _guided_ref as GR
import _parity
from oracle import ref_cpu as R

T = 100
TAUS = [25, 50, 75, 100]


def _bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def _case(n=2, H=16, f=4, seed=5, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, H, H, generator=g).to(dtype)
    obs = torch.randn(n, H // f, H // f, generator=g)
    wgt = torch.rand(n, H // f, H // f, generator=g)
    wgt[0, 0, :2] = 0
    return x, obs, wgt, g


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_adjoint_identity(f):
    """<A v, q> == <v, A^T q> in fp64 for the restatement's block mean and its spread."""
    g = torch.Generator().manual_seed(f)
    v = torch.randn(3, 16, 16, generator=g, dtype=torch.float64)
    q = torch.randn(3, 16 // f, 16 // f, generator=g, dtype=torch.float64)
    lhs, rhs = (GR.block_mean(v, f) * q).sum().item(), (v * GR.block_mean_T(q, f)).sum().item()
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1.0)


def _stand_in(g):
    """A small differentiable stand-in for eps: a fixed random 3x3 conv plus tanh."""
    k = torch.randn(1, 1, 3, 3, generator=g, dtype=torch.float64) * 0.4
    return lambda x: torch.tanh(torch.nn.functional.conv2d(x[:, None], k, padding=1))[:, 0]


@pytest.mark.parametrize("f", [1, 4])
def test_restatement_gradient_vs_autograd_and_fd(f):
    """grad = gdir + (VJP of deps through eps) equals fp64 autograd of L through x0h(x, eps(x)) to 1e-12, and a central
    finite difference to the accuracy the difference allows: |fd - grad . d| is measured for h = 1e-5 and recorded; its
    bound is the truncation h^2 |L'''| / 6 plus the rounding eps L / h, here taken as 1e-6 relative."""
    x, obs, wgt, g = _case(f=f)
    net = _stand_in(g)
    sq, ra = (t[2] for t in GR.tables(R.make_schedule(T)[2], TAUS, torch.float64))

    def loss(xx):
        x0h = (xx - sq * net(xx)) * ra
        r = obs.double() - GR.block_mean(x0h, f)
        return (wgt.double() * r * r).sum()

    xin = x.clone().requires_grad_(True)
    auto = torch.autograd.grad(loss(xin), xin)[0]
    xin = x.clone().requires_grad_(True)
    eps = net(xin)
    o = GR.residual_grad(x, eps.detach(), None, 0.0, obs, wgt, f, sq, ra)
    grad = o["gdir"] + torch.autograd.grad((eps * o["deps_c"]).sum(), xin)[0]
    assert abs(o["L"].sum().item() - loss(x).item()) <= 1e-12 * loss(x).item()
    err = ((grad - auto).norm() / auto.norm()).item()
    d = torch.randn(x.shape, generator=g, dtype=torch.float64)
    h = 1e-5
    fd = ((loss(x + h * d) - loss(x - h * d)) / (2 * h)).item()
    an = (auto * d).sum().item()
    fd_err = abs(fd - an) / abs(an)
    print(f"[guided restatement f={f}] autograd rel {err:.3e}; central FD (h = {h}) rel {fd_err:.3e}")
    _parity.record("guided_restatement_grad", f=f, autograd_rel=err, fd_rel=fd_err, fd_h=h)
    assert err <= 1e-12
    assert fd_err <= 1e-6


def test_guided_tables_closed_forms():
    from cdm_amd.diffusion import guided_tables
    ab = R.make_schedule(T)[2]
    sq, ra = guided_tables(ab, TAUS)
    assert sq.dtype == np.float32 and sq.shape == ra.shape == (len(TAUS) + 1,)
    ab64 = ab.double().numpy()
    want_sq = np.concatenate([[0.0], np.sqrt(1 - ab64[TAUS])]).astype(np.float32)
    want_ra = np.concatenate([[1.0], 1 / np.sqrt(ab64[TAUS])]).astype(np.float32)
    assert sq.tobytes() == want_sq.tobytes() and ra.tobytes() == want_ra.tobytes()
    rsq, rra = GR.tables(ab, TAUS)
    assert _bits(torch.from_numpy(sq), rsq) and _bits(torch.from_numpy(ra), rra)
    with pytest.raises(ValueError):
        guided_tables(ab, [50, 25, 100])
    with pytest.raises(ValueError):
        guided_tables(torch.zeros(T + 1), TAUS)


def test_check_observation_errors():
    from cdm_amd.diffusion import check_observation
    n, H = 2, 16
    obs, wgt = torch.zeros(n, 1, 4, 4), torch.ones(1, 1, 4, 4)
    o, w = check_observation(obs, None, n, H, 4, 1.0, 1)
    assert tuple(o.shape) == (n, 1, 4, 4) and tuple(w.shape) == (1, 1, 4, 4) and bool((w == 1).all())
    assert tuple(check_observation(obs[:, 0], wgt[:, 0], n, H)[0].shape) == (n, 1, 4, 4)
    nan_ok = obs.clone(); nan_ok[0, 0, 0, 0] = float("nan")
    hole = torch.ones(n, 1, 4, 4); hole[0, 0, 0, 0] = 0
    check_observation(nan_ok, hole, n, H)                                   # unobserved cells may hold anything
    bad = [
        dict(obs=torch.zeros(n, 1, 8, 8)), dict(obs=torch.zeros(n + 1, 1, 4, 4)), dict(obs=torch.zeros(n, 2, 4, 4)),
        dict(obs=None), dict(weight=torch.ones(3, 1, 4, 4)), dict(weight=torch.ones(1, 1, 8, 8)),
        dict(factor=3), dict(factor=16), dict(factor=True), dict(factor=8, H=20, obs=torch.zeros(n, 1, 2, 2)),
        dict(weight=-wgt), dict(weight=wgt * float("nan")), dict(weight=wgt * float("inf")),
        dict(zeta=-0.1), dict(zeta=float("nan")), dict(zeta=float("inf")), dict(in_channels=2),
        dict(obs=nan_ok), dict(obs=torch.zeros(n, 1, 4, 4, dtype=torch.int32)),
    ]
    for kw in bad:
        a = dict(obs=obs, weight=wgt, n=n, H=H, factor=4, zeta=1.0, in_channels=1)
        a.update(kw)
        with pytest.raises(ValueError):
            check_observation(**a)


@pytest.mark.parametrize("cfg", [False, True])
def test_zeta_zero_is_the_ddim_restatement(cfg):
    x, obs, wgt, g = _case(dtype=torch.float32)
    ec, eu = torch.randn(x.shape, generator=g), (torch.randn(x.shape, generator=g) if cfg else None)
    z = torch.randn(x.shape, generator=g)
    cx, ce, sg = (t[3] for t in D.coefficients(R.make_schedule(T)[2], TAUS, 0.7))
    w = torch.tensor(1.5)
    got = GR.guided_update(x, ec, eu, 1.5, cx, ce, sg, z, None, None, None, torch.ones(2, dtype=torch.float64), 0.0)
    assert _bits(got, D.step(x, ec, eu, w, cx, ce, sg, z))
    # an L == 0 sample keeps the DDIM step's bits at zeta > 0 too
    gd = torch.randn(x.shape, generator=g)
    got = GR.guided_update(x, ec, eu, 1.5, cx, ce, sg, z, gd, gd, gd if cfg else None,
                           torch.tensor([0.0, 2.0], dtype=torch.float64), 0.5)
    want = D.step(x, ec, eu, w, cx, ce, sg, z)
    assert _bits(got[0], want[0]) and not _bits(got[1], want[1])


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_closing_row_is_the_weighted_norm(f):
    x, obs, wgt, _ = _case(H=16, f=f)
    got = GR.closing_L(x, obs, wgt, f).sqrt()
    pooled = torch.nn.functional.avg_pool2d(x[:, None], f)[:, 0]
    want = (wgt.double().sqrt() * (obs.double() - pooled)).flatten(1).norm(dim=1)
    assert torch.allclose(got, want, rtol=1e-13, atol=0)


def test_fold_sum_is_a_sum():
    t = np.random.default_rng(0).random(1000)
    assert abs(GR.fold_sum(t) - t.sum()) <= 1e-12 * t.sum()
    assert GR.fold_sum(np.zeros(5)) == 0.0


def test_degrade():
    from cdm_amd.diffusion import degrade
    m = torch.rand(2, 1, 16, 16)
    assert _bits(degrade(m, 4), torch.nn.functional.avg_pool2d(m, 4))
    a, b = degrade(m, 4, 0.1, seed=3), degrade(m[:, 0], 4, 0.1, seed=3)
    assert _bits(a, b) and tuple(a.shape) == (2, 1, 4, 4) and not _bits(a, degrade(m, 4, 0.1, seed=4))
    for kw in (dict(factor=3), dict(factor=4, sigma=-1.0)):
        with pytest.raises(ValueError):
            degrade(m, **kw)


def test_cli_argument_errors(tmp_path, capsys):
    """The --observe flags are checked while the arguments are parsed, before any device work: argparse errors (exit 2)."""
    cli_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camels-diffusion-model_amd",
                            "train_diffusion.py")
    spec = importlib.util.spec_from_file_location("_train_diffusion_cli", cli_path)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    op, wp = str(tmp_path / "obs.npy"), str(tmp_path / "wgt.npy")
    np.save(op, np.zeros((2, 16, 16), dtype=np.float32)); np.save(wp, -np.ones((16, 16), dtype=np.float32))
    base = ["1e-3", "1", "20", "--synthetic", "8", "--n-samples", "2", "--out-root", str(tmp_path / "out")]
    for extra, needle in ((["--observe", op, "--sample-steps", "4"], "--observe-factor"),
                          (["--observe", op, "--observe-factor", "4"], "--sample-steps"),
                          (["--observe-factor", "4", "--sample-steps", "4"], "need --observe"),
                          (["--observe", op, "--observe-factor", "8", "--sample-steps", "4"], "obs must have shape"),
                          (["--observe", op, "--observe-factor", "3", "--sample-steps", "4"], "factor must be"),
                          (["--observe", op, "--observe-factor", "4", "--sample-steps", "4", "--sampler", "dpmpp"], "DDIM"),
                          (["--observe", op, "--observe-factor", "4", "--sample-steps", "4", "--observe-weight", wp],
                           "weight values"),
                          (["--observe", op, "--observe-factor", "4", "--sample-steps", "4", "--observe-zeta", "-1"],
                           "zeta")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert needle in err, (extra, err)
    assert not (tmp_path / "out").exists()
