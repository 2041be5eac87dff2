"""Host side of DDIM encoding and the flow likelihood (cdm_amd.encode / log_likelihood): the encoding tables, the
definition on a closed-form Gaussian (where the log-density is known exactly), the restatement the GPU tests compare
against (tests/_flow_ref.py) checked against an explicit Jacobian, argument validation, ScanResult.from_logp.  No GPU."""
import math

import numpy as np
import pytest
import torch

import cdm_amd
import _ddim_ref as D
import _flow_ref as FL
import _parity
from cdm_amd import ScanResult, check_flow, encode_tables
from oracle import ref_cpu as R


# ----------------------------------------------------------------------------------------------------------------------
# encode_tables
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,spacing", [(100, 4, "uniform"), (1500, 25, "quadratic"), (50, 50, "uniform"),
                                         (1500, 1, "uniform")])
def test_encode_tables_invert_the_ddim_step(T, S, spacing):
    """In fp64, before rounding: ix cx = 1, ie = -ce / cx, g = -ce against the fp64 restatement of ddim_tables
    (tests/_ddim_ref.coefficients at eta = 0); the committed tables are those values rounded once (ix, ie: fp32; g kept
    fp64); from_t is taus ascending in run order (position p = S..1 performs step S + 1 - p); entry 0 is the identity."""
    ab = R.make_schedule(T)[2]
    taus = D.subsequence(T, S, spacing)
    from_t, ix, ie, g = encode_tables(ab, taus)
    assert from_t.dtype == np.int32 and ix.dtype == np.float32 and ie.dtype == np.float32 and g.dtype == np.float64
    assert all(v.shape == (S + 1,) for v in (from_t, ix, ie, g))
    assert (from_t[0], ix[0], ie[0], g[0]) == (0, 1.0, 0.0, 0.0)
    assert [int(from_t[p]) for p in range(S, 0, -1)] == taus and int(from_t[1]) == T
    cx, ce, _ = (v.numpy() for v in D.coefficients(ab, taus, 0.0, torch.float64))
    rix, rie, rg = (v.numpy() for v in FL.coefficients(ab, taus, torch.float64))
    for k in range(1, S + 1):
        p = S + 1 - k
        assert abs(rix[k] * cx[k] - 1) <= 4e-16 and abs(rie[k] + ce[k] / cx[k]) <= 4e-16 * abs(rie[k])
        assert rg[k] == -ce[k]
        assert abs(g[p] - rg[k]) <= 4e-16 * abs(rg[k]) and g[p] > 0
        assert ix[p] == np.float32(rix[k]) or abs(float(ix[p]) - rix[k]) <= 2 ** -24 * rix[k]
        assert abs(float(ie[p]) - rie[k]) <= 2 ** -24 * abs(rie[k])
        assert abs(float(ie[p]) / float(ix[p]) - g[p]) <= 3 * 2 ** -24 * g[p]          # g = ie / ix


def test_encode_tables_errors():
    ab = R.make_schedule(20)[2]
    for taus in ([], [0, 20], [5, 5, 20], [5, 10], [5, 30], [2.5, 20], [10, 5, 20]):
        with pytest.raises(ValueError):
            encode_tables(ab, taus)
    bad = ab.clone(); bad[20] = 0.0
    with pytest.raises(ValueError, match="non-finite"):
        encode_tables(bad, [10, 20])
    bad = ab.clone(); bad[10] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        encode_tables(bad, [10, 20])


# ----------------------------------------------------------------------------------------------------------------------
# the definition on a closed-form Gaussian
# ----------------------------------------------------------------------------------------------------------------------
GT, GH = 1500, 4                       # D = 16
_GAUSS = {}


def _gauss_error(s2, S, spacing, form):
    """mean over 8 maps x_0 ~ N(0, s2 I) of (walk's logp - log N(x_0; 0, s2 I)), fp64, walked with the product's
    encode_tables (ix, ie as rounded to fp32, g fp64; position p = S + 1 - k); J = c I, so the probe is exact."""
    key = (s2, S, spacing, form)
    if key not in _GAUSS:
        ab = R.make_schedule(GT)[2]
        taus = D.subsequence(GT, S, spacing)
        g = torch.Generator().manual_seed(5)
        x0 = math.sqrt(s2) * torch.randn(8, GH, GH, generator=g, dtype=torch.float64)
        v = FL.probe_from_uniform(torch.rand(GH, GH, generator=g))
        by_step = tuple(torch.from_numpy(np.concatenate([t[:1], t[:0:-1]]).astype(np.float64))
                        for t in encode_tables(ab, taus)[1:])
        out = FL.walk(FL.gaussian_eps(ab, taus, s2), x0, ab, taus, torch.float64, [v] * S, form, tables=by_step)
        assert not bool(out["invalid"].any())
        # the probe is exact here: q = c D whatever v
        c = torch.tensor([float(FL.gaussian_eps(ab, taus, s2)(torch.ones(1, dtype=torch.float64), k)) for k in range(1, S + 1)], dtype=torch.float64)
        assert torch.allclose(out["q"], (c * GH * GH)[:, None].expand(S, 8), rtol=1e-12, atol=0)
        _GAUSS[key] = float((out["logp"] - FL.gaussian_logp(x0, s2)).mean())
    return _GAUSS[key]


@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_gaussian_trace_form_is_first_order(s2):
    """form="trace": the error against the exact log-density halves on doubling S, S = 50 -> 100 -> 200 -> 400: each
    ratio in [1.8, 2.3]."""
    errs = [_gauss_error(s2, S, "uniform", "trace") for S in (50, 100, 200, 400)]
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    print(f"[flow gaussian trace s2={s2}] errors {errs} ratios {ratios}")
    _parity.record("flow_gaussian_trace", s2=s2, S=[50, 100, 200, 400], error_nats=errs, ratios=ratios,
                   error_S25=_gauss_error(s2, 25, "uniform", "trace"))
    assert all(1.8 <= r <= 2.3 for r in ratios), (s2, errs, ratios)


@pytest.mark.parametrize("spacing", ["uniform", "quadratic"])
@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_gaussian_logdet_form(s2, spacing):
    """form="logdet": |error| / D <= 0.02 nats at S = 25, 50, 100, 200, 400."""
    Ss = (25, 50, 100, 200, 400)
    errs = [_gauss_error(s2, S, spacing, "logdet") for S in Ss]
    per_dim = [abs(e) / (GH * GH) for e in errs]
    print(f"[flow gaussian logdet s2={s2} {spacing}] errors {errs} per dimension {per_dim}")
    _parity.record("flow_gaussian_logdet", s2=s2, spacing=spacing, S=list(Ss), error_nats=errs, per_dim=per_dim)
    assert max(per_dim) <= 0.02, (s2, spacing, errs)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement against an explicit Jacobian; its log1p against libm's
# ----------------------------------------------------------------------------------------------------------------------
def _tiny_sd(nf, ncf, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape, kind in R.state_dict_layout(1, nf, ncf, H):
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)
        else:
            fan = max(1, int(np.prod(shape[1:]))) if len(shape) > 1 else 1
            sd[k] = torch.randn(shape, generator=g, dtype=torch.float64) / math.sqrt(fan) + (1.0 if len(shape) == 1 and
                                                                                             ".1.weight" in k else 0.0)
    return sd


def test_restatement_q_equals_explicit_jacobian():
    """On a tiny oracle model (H = 8, D = 64) the restatement's q for a given v equals v^T J v with J from
    torch.autograd.functional.jacobian in fp64, to 1e-10 relative; so does its dx against J^T v."""
    nf, ncf, H, T = 8, 6, 8, 20
    sd = _tiny_sd(nf, ncf, H)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, H, H, generator=g, dtype=torch.float64)
    c = torch.rand(2, ncf, generator=g, dtype=torch.float64)
    v = FL.probe_from_uniform(torch.rand(H, H, generator=g)).double()
    rows = [[(torch.randn(nf, 1, 1, 1, generator=g, dtype=torch.float64), torch.randn(nf, generator=g, dtype=torch.float64))]]
    eps_fn = FL.oracle_eps(sd, c, 0.0, T, [T], rows, torch.float64, n_feat=nf, n_cfeat=ncf, height=H)
    xin = x.clone().requires_grad_(True)
    q, dx = FL.vjp_q(eps_fn(xin, 1), xin, v)
    for s in range(2):
        f = lambda xs: eps_fn(torch.cat([x[:s], xs[None], x[s + 1:]]), 1)[s]    # noqa: E731  (eval mode: rows independent)
        J = torch.autograd.functional.jacobian(f, x[s]).reshape(H * H, H * H)
        want = v.reshape(-1) @ J @ v.reshape(-1)
        rel = abs(float(q[s] - want)) / abs(float(want))
        rel_dx = float((dx[s].reshape(-1) - J.T @ v.reshape(-1)).norm() / (J.T @ v.reshape(-1)).norm())
        _parity.record("flow_restatement_vs_jacobian", row=s, q=float(q[s]), rel=rel, rel_dx=rel_dx, trace=float(J.trace()))
        assert rel <= 1e-10 and rel_dx <= 1e-10, (s, float(q[s]), float(want))


def test_restated_log1p_against_libm():
    """The kernel's IEEE-only log1p (restated line by line in _flow_ref.log1p_ieee) against math.log1p over the whole
    range a row can reach: within 4 ulp (|result| >= 1e-300), exact 0 at 0."""
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(-0.999999, 3.0, 4000), 10.0 ** rng.uniform(-18, 3, 2000),
                        -(10.0 ** rng.uniform(-18, -0.001, 2000)), [0.0, -0.2928, 0.4142, 1e-300, -1 + 2.0 ** -53, 1e300]])
    worst = 0.0
    for v in a:
        got, want = float(FL.log1p_ieee(v)), math.log1p(v)
        worst = max(worst, abs(got - want) / np.spacing(abs(want)) if want != 0 else abs(got))
    _parity.record("flow_log1p_ieee_vs_libm", worst_ulp=worst, n=int(a.size))
    assert worst <= 4, worst
    assert float(FL.log1p_ieee(0.0)) == 0.0
    assert math.isnan(float(FL.ld_term(-70.0, 64, "logdet"))) and math.isnan(float(FL.ld_term(-64.0, 64, "logdet")))
    assert float(FL.ld_term(-70.0, 64, "trace")) == -70.0


# ----------------------------------------------------------------------------------------------------------------------
# check_flow, the argument checks of the public interface, ScanResult.from_logp
# ----------------------------------------------------------------------------------------------------------------------
NCF, H = 6, 64


def test_check_flow_accepts_and_normalises():
    maps = np.random.default_rng(0).random((3, H, H)).astype(np.float32)
    x, c = check_flow(maps, torch.rand(3, NCF), NCF, H)
    assert tuple(x.shape) == (3, 1, H, H) and tuple(c.shape) == (3, NCF)
    x, c = check_flow(torch.rand(2, 1, H, H), None, NCF, H, form="trace", n_probe=4, max_rows=1)
    assert tuple(x.shape) == (2, 1, H, H) and c is None


@pytest.mark.parametrize("kw", [
    dict(guide_w=2.0), dict(guide_w=-1.0), dict(guide_w=float("nan")), dict(in_channels=2), dict(form="exact"),
    dict(form=None), dict(n_probe=0), dict(n_probe=1.5), dict(n_probe=True), dict(max_rows=0),
    dict(maps=torch.zeros(2, H, H - 1)), dict(maps=torch.zeros(2, 2, H, H)), dict(maps=torch.zeros(0, 1, H, H)),
    dict(maps=torch.zeros(H, H)), dict(maps=torch.zeros(2, H, H, dtype=torch.int32)),
    dict(maps=torch.full((2, H, H), float("nan"))), dict(params=torch.zeros(3, NCF)), dict(params=torch.zeros(2, NCF + 1)),
    dict(params=torch.zeros(NCF)), dict(params=torch.full((2, NCF), float("inf"))),
])
def test_check_flow_errors(kw):
    args = dict(maps=torch.rand(2, 1, H, H), params=torch.rand(2, NCF), n_cfeat=NCF, H=H)
    with pytest.raises(ValueError):
        check_flow(**{**args, **kw})


def test_scan_result_from_logp():
    logp = torch.tensor([[-10.0, -8.0, -11.0], [-3.0, -3.0, -5.0]], dtype=torch.float64)
    cand = torch.tensor([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    r = ScanResult.from_logp(logp, cand)
    assert torch.equal(r.score, -logp) and r.t_grid == [] and r.weight == "logp"
    assert torch.equal(r.log_weights(1), logp - logp.max(1, keepdim=True).values)
    mean, std, w = r.posterior(1)
    assert torch.allclose(w, torch.softmax(logp, 1)) and torch.allclose(mean, torch.softmax(logp, 1) @ cand.double())
    assert r.best_index().tolist() == [1, 0] and torch.equal(r.best(), cand[[1, 0]])
    for bad in (dict(logp=logp[0]), dict(candidates=cand[:2]), dict(logp=torch.full((2, 3), float("nan")))):
        with pytest.raises(ValueError):
            ScanResult.from_logp(**{**dict(logp=logp, candidates=cand), **bad})


def test_run_keys_do_not_collide_across_neighbouring_seeds():
    """flow_run_key = the restated splitmix64 chain; the keys of seeds 0..63 x runs 0..7 are all distinct (seed ^ r would
    share most of them); 64-bit values."""
    keys = {(s, r): cdm_amd.flow_run_key(s, r) for s in range(64) for r in range(8)}
    assert all(k == FL.run_key(s, r) and 0 <= k < 2 ** 64 for (s, r), k in keys.items())
    assert len(set(keys.values())) == len(keys)
    assert cdm_amd.flow_run_key(2 ** 63 - 1, 3) == FL.run_key(2 ** 63 - 1, 3)


def test_public_names():
    for name in ("encode", "log_likelihood", "DDIMEncoder", "FlowLikelihood", "FlowResult", "encode_tables", "check_flow"):
        assert name in cdm_amd.__all__ and hasattr(cdm_amd, name)
    assert hasattr(cdm_amd.DDPM, "encode") and hasattr(cdm_amd.DDPM, "log_likelihood")
