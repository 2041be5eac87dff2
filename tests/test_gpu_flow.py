"""DDIM encoding and the flow likelihood on the captured step graph: the three kernels bit for bit against
tests/_flow_ref.py, their argument checks, DDPM.encode and one position's q against the fp64 restatement on the oracle's
forward, the whole log_likelihood against the restatement run with the kernel's probes, row / seed / chunk determinism,
graph replay, and the round trip (recorded).

Model: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64) in eval mode with randomised BatchNorm running
statistics; T = 100, S = 4, n = 2.  The bar of every comparison with fp64 is the project's: relative L2 <= 3 x the fp32
restatement's own deviation from fp64 + 2e-6; every figure is printed and recorded before it is asserted.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
import _flow_ref as FL
import _parity
from _kinks import Kinks
from _flow_gpu_common import (H, KW, N, NCF, NF, S, T, ab as _ab, bits as _bits, draws as _draws, half as _half,
                              hip_kinks_split as _hip_kinks_split, i32 as _i32, model as _model, ptr as _ptr,
                              rel_l2 as _rel_l2, sd as _sd, stream as _stream, taus as _taus)

pytestmark = pytest.mark.gpu
INVALID = 1          # hipErrorInvalidValue
DOMAIN = 0x666C6F7770726F62          # the probe's key domain (csrc/sampler_parts.h)
RUN_SEED = 4321
SEED = 77          # of the CPU RNG before a walk draws its shortcut rows


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _problem(seed=3, n=N):
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn(n, 1, H, H, generator=g), torch.rand(n, NCF, generator=g)


def _kernel_probe(h, p, npos, seed, run, n=1):
    """cdm_flow_probe's v [n, h, h] at the position p under the run key seed ^ run (run: any 64-bit value)."""
    from cdm_amd._lib import lib
    v = torch.full((n, h, h), 7.0).cuda()
    zs = torch.tensor([run - (1 << 64) if run >> 63 else run], dtype=torch.int64).cuda()
    cur = _i32([p])
    lib().cdm_flow_probe(_ptr(v), n, h, _ptr(cur), npos, seed, _ptr(zs), _stream())
    torch.cuda.synchronize()
    return v.cpu()


# ---------------------------------------------------------------------------------------------------------------
# 1. cdm_flow_probe
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [8, 24])
def test_probe_kernel(h):
    """Bit for bit cdm_philox_uniform(out, h h, 0, 1, key, sub = p) thresholded at 0.5, key = (seed ^ run) ^ the probe's
    domain, at the positions 1 and S; identical across rows; different between two run keys and between positions; a
    position outside 1..npos writes nothing."""
    from cdm_amd._lib import lib
    lb = lib()
    n, npos, seed = 3, S, 1234
    got = {}
    for run in (0, 1):
        for p in (1, npos):
            v = _kernel_probe(h, p, npos, seed, run, n)
            u = torch.empty(h * h).cuda()
            lb.cdm_philox_uniform(_ptr(u), h * h, 0.0, 1.0, (seed ^ run) ^ DOMAIN, p, None, _stream())
            torch.cuda.synchronize()
            want = FL.probe_from_uniform(u.cpu()).reshape(h, h)
            assert all(_bits(v[b], want) for b in range(n)), (h, run, p)
            assert bool((v.abs() == 1).all())
            got[run, p] = v
    assert not _bits(got[0, 1], got[1, 1]) and not _bits(got[0, 1], got[0, npos])
    assert 0.3 < float((got[0, 1] > 0).float().mean()) < 0.7
    for p in (0, npos + 1):
        assert bool((_kernel_probe(h, p, npos, seed, 0, n) == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# 2. cdm_flow_step and cdm_flow_finish, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("form", ["trace", "logdet"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h", [8, 24])
def test_step_and_finish_kernels_bit_exact(h, n, form, off):
    """x, q (the hist row), acc and invalid = tests/_flow_ref.flow_step, prior and logp = _flow_ref.finish (the fp64 sums
    in the kernel's order, the kernel's log1p restated: exact bits are asked for), at two positions, from buffers offset
    by ``off`` floats; a second step accumulates onto the first; a position outside the range leaves every output
    untouched."""
    from cdm_amd._lib import lib
    lb = lib()
    npos, seed, run = 5, 99, 2
    g = torch.Generator().manual_seed(1000 * h + 10 * n + off)
    x, eps, dx = (torch.randn(n, h, h, generator=g) for _ in range(3))
    dx = dx * 0.3
    ix, ie = 0.5 + torch.rand(npos + 1, generator=g), torch.rand(npos + 1, generator=g)
    gt = 0.2 + torch.rand(npos + 1, generator=g, dtype=torch.float64)
    zs = torch.tensor([run], dtype=torch.int64).cuda()

    def shifted(t):
        buf = torch.zeros(t.numel() + off).cuda()
        view = buf[off:].view(t.shape)
        view.copy_(t)
        return view
    xd, ed, dd = shifted(x), shifted(eps), shifted(dx)
    ixd, ied, gd = shifted(ix), shifted(ie), gt.cuda()
    acc = torch.zeros(n, dtype=torch.float64).cuda()
    hist = torch.full((npos + 1, n), -7.0, dtype=torch.float64).cuda()
    inv = torch.zeros(n, dtype=torch.int32).cuda()
    fi = FL.FORMS.index(form)
    want_x, want_acc = x, np.zeros(n)
    for p in (npos, 2):
        v = _kernel_probe(h, p, npos, seed, run)[0]
        want_x, q, want_acc, bad = FL.flow_step(want_x, eps, dx, v, ix[p], ie[p], float(gt[p]), form, want_acc)
        cur = _i32([p])
        lb.cdm_flow_step(_ptr(xd), _ptr(ed), _ptr(dd), n, h, _ptr(cur), _ptr(ixd), _ptr(ied), _ptr(gd), npos, fi,
                         seed, _ptr(zs), _ptr(acc), _ptr(hist), _ptr(inv), _stream())
        torch.cuda.synchronize()
        assert _bits(xd.cpu(), want_x), (h, n, form, off, p)
        assert _bits(hist[p].cpu(), torch.from_numpy(q)), (hist[p].cpu(), q)
        assert _bits(acc.cpu(), torch.from_numpy(want_acc)), (acc.cpu(), want_acc)
        assert not bad.any() and not bool(inv.any())
    assert bool((hist[[r for r in range(npos + 1) if r not in (npos, 2)]] == -7.0).all())
    prior, logp = (torch.full((n,), -7.0, dtype=torch.float64).cuda() for _ in range(2))
    lb.cdm_flow_finish(_ptr(xd), n, h, -3.25, _ptr(acc), _ptr(prior), _ptr(logp), _stream())
    torch.cuda.synchronize()
    wp, wl = FL.finish(want_x, -3.25, want_acc)
    assert _bits(prior.cpu(), torch.from_numpy(wp)) and _bits(logp.cpu(), torch.from_numpy(wl))
    before = [t.clone() for t in (xd, acc, hist, inv)]
    for p in (0, npos + 1, -2):
        cur = _i32([p])
        lb.cdm_flow_step(_ptr(xd), _ptr(ed), _ptr(dd), n, h, _ptr(cur), _ptr(ixd), _ptr(ied), _ptr(gd), npos, fi,
                         seed, _ptr(zs), _ptr(acc), _ptr(hist), _ptr(inv), _stream())
        torch.cuda.synchronize()
    assert all(_bits(a.cpu(), b.cpu()) for a, b in zip((xd, acc, hist, inv), before))


def test_step_kernel_invalid_rows():
    """A row with 1 + g q / D <= 0 (logdet: NaN; trace: finite, not flagged) and a row whose dx holds a NaN set their own
    ``invalid`` and acc and nothing in the other rows."""
    from cdm_amd._lib import lib
    lb = lib()
    h, n, npos, seed, p = 8, 4, 3, 5, 2
    Dn = h * h
    v = _kernel_probe(h, p, npos, seed, 0)[0]
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(n, h, h, generator=g), torch.randn(n, h, h, generator=g)
    dx = 0.1 * torch.randn(n, h, h, generator=g)
    dx[1] = -2.0 * v                      # q = -2 D, g = 1: 1 + g q / D = -1
    dx[2, 3, 3] = float("nan")
    ix, ie, gt = torch.ones(npos + 1), torch.full((npos + 1,), 0.5), torch.ones(npos + 1, dtype=torch.float64)
    zs = torch.zeros(1, dtype=torch.int64).cuda()
    for form in FL.FORMS:
        xd, acc = x.clone().cuda(), torch.zeros(n, dtype=torch.float64).cuda()
        hist, inv = torch.zeros(npos + 1, n, dtype=torch.float64).cuda(), torch.zeros(n, dtype=torch.int32).cuda()
        ed, dd, ixd, ied, gd, cur = eps.cuda(), dx.cuda(), ix.cuda(), ie.cuda(), gt.cuda(), _i32([p])
        lb.cdm_flow_step(_ptr(xd), _ptr(ed), _ptr(dd), n, h, _ptr(cur), _ptr(ixd), _ptr(ied), _ptr(gd), npos,
                         FL.FORMS.index(form), seed, _ptr(zs), _ptr(acc), _ptr(hist), _ptr(inv), _stream())
        torch.cuda.synchronize()
        wx, q, wacc, bad = FL.flow_step(x, eps, dx, v, ix[p], ie[p], 1.0, form, np.zeros(n))
        assert q[1] == -2.0 * Dn
        assert inv.cpu().tolist() == [0, int(form == "logdet"), 1, 0] == [int(b) for b in bad]
        got = acc.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(wacc)) and _bits(xd.cpu(), wx)
        assert got[~np.isnan(got)].tobytes() == wacc[~np.isnan(wacc)].tobytes()
        assert bool(torch.isfinite(acc.cpu()[[0, 3]]).all()) and bool(torch.isnan(acc.cpu()[2]))


def test_invalid_arguments_write_nothing():
    from cdm_amd._lib import lib
    lb = lib()
    n, h, npos = 2, 8, 3
    F32 = lambda *sh: torch.full(sh, 5.0).cuda()                            # noqa: E731
    F64 = lambda *sh: torch.full(sh, 5.0, dtype=torch.float64).cuda()       # noqa: E731
    x, eps, dx, tab, g = F32(n, h, h), F32(n, h, h), F32(n, h, h), F32(npos + 1), F64(npos + 1)
    acc, hist, prior, logp, inv = F64(n), F64(npos + 1, n), F64(n), F64(n), torch.full((n,), 5, dtype=torch.int32).cuda()
    cur = _i32([2])
    good = dict(v=_ptr(x), n=n, H=h, cur_k=_ptr(cur), npos=npos, seed=1, seed_dev=None, stream=_stream())
    for kw in (dict(v=None), dict(cur_k=None), dict(n=0), dict(H=0), dict(npos=0)):
        assert lb.raw("cdm_flow_probe")(*{**good, **kw}.values()) == INVALID, kw
    good = dict(x=_ptr(x), eps=_ptr(eps), dx=_ptr(dx), n=n, H=h, cur_k=_ptr(cur), ix=_ptr(tab), ie=_ptr(tab), g=_ptr(g),
                npos=npos, form=1, seed=1, seed_dev=None, acc=_ptr(acc), hist=_ptr(hist), invalid=_ptr(inv),
                stream=_stream())
    for kw in (dict(x=None), dict(eps=None), dict(dx=None), dict(cur_k=None), dict(ix=None), dict(ie=None), dict(g=None),
               dict(acc=None), dict(hist=None), dict(invalid=None), dict(n=0), dict(H=0), dict(npos=0), dict(form=2),
               dict(form=-1)):
        assert lb.raw("cdm_flow_step")(*{**good, **kw}.values()) == INVALID, kw
    good = dict(x=_ptr(x), n=n, H=h, log_abT=-1.0, acc=_ptr(acc), prior=_ptr(prior), logp=_ptr(logp), stream=_stream())
    for kw in (dict(x=None), dict(acc=None), dict(prior=None), dict(logp=None), dict(n=0), dict(H=0), dict(log_abT=0.5),
               dict(log_abT=float("nan")), dict(log_abT=float("-inf"))):
        assert lb.raw("cdm_flow_finish")(*{**good, **kw}.values()) == INVALID, kw
    torch.cuda.synchronize()
    for t in (x, eps, dx, acc, hist, prior, logp, inv):
        assert bool((t == 5).all())


# ---------------------------------------------------------------------------------------------------------------
# 3. DDPM.encode against the fp64 restatement; graph replay
# ---------------------------------------------------------------------------------------------------------------
def _rows_by_step(sets):
    """The shortcut draws after torch.manual_seed(SEED), in the walk's order: rows[k - 1] = those of step k."""
    return _draws(SEED, 0.0, sets)[0]


_ENC = {}


def _ref_encode(w):
    if w not in _ENC:
        x0, params = _problem()
        rows = _rows_by_step(2 if w > 0 else 1)
        _ENC[w] = tuple(FL.walk(FL.oracle_eps(_sd(), params, w, T, _taus(), rows, dt, **KW), x0[:, 0], _ab(), _taus(),
                                dt)["x"] for dt in (torch.float32, torch.float64))
    return _ENC[w]


@pytest.mark.parametrize("math", ["h3", "fp32"])
@pytest.mark.parametrize("w", [0.0, 2.0])
def test_encode_vs_fp64(math, w):
    import cdm_amd
    x0, params = _problem()
    x32, x64 = _ref_encode(w)
    d = cdm_amd.DDPM(_model(math), T)
    torch.manual_seed(SEED)
    xT, inter = d.encode(x0, params, guide_w=w, steps=S, save_rate=2)
    assert tuple(xT.shape) == (N, 1, H, H) and xT.is_cuda and inter.shape == (S, N, 1, H, H)
    assert np.array_equal(inter[-1], xT.cpu().numpy())
    e, er = _rel_l2(xT[:, 0], x64), _rel_l2(x32, x64)
    print(f"[flow encode {math} w={w}] hip {e:.3e} ref32 {er:.3e} ratio {e / (3 * er + 2e-6):.2f}")
    _parity.record("flow_encode", math=math, w=w, hip=e, ref32=er, ratio=e / (3 * er + 2e-6))
    assert e <= 3 * er + 2e-6, (math, w, e, er)


@pytest.mark.parametrize("w", [0.0, 2.0])
def test_encode_graph_replay_equals_eager(w):
    import cdm_amd
    m = _model("fp32")
    x0, params = _problem()
    d = cdm_amd.DDPM(m, T)
    out = []
    for kw in (dict(steps_per_graph=2), dict(use_graph=False)):
        smp = cdm_amd.DDIMEncoder(m, d.sched, N, w, params, steps=S, save_rate=2, **kw)
        torch.manual_seed(SEED)
        smp.prepare_rng(host_z=False)
        out.append(smp.run(x0))
        assert (smp.graph is not None) == ("steps_per_graph" in kw)
    assert _bits(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------
# 4. one position's q against fp64 autograd on HIP's own branch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_one_position_q_vs_fp64(math):
    """q of the first position (step 1, p = S) against fp64 autograd of the restatement on HIP's own ReLU / MaxPool
    branch; the fp32 restatement against fp64 on its own branch gives the bar."""
    import cdm_amd
    m = _model(math)
    x0, params = _problem()
    taus, ab = _taus(), _ab()
    rows = _rows_by_step(1)
    d = cdm_amd.DDPM(m, T)
    smp = cdm_amd.FlowLikelihood(m, d.sched, N, params, steps=S, use_graph=False, seed=RUN_SEED)
    torch.manual_seed(SEED)
    smp.prepare_rng(host_z=False)
    res = smp.run(x0, 1, steps=1)
    q_hip = res["hist"][0, 0]
    v = _kernel_probe(H, S, S, 0, FL.run_key(RUN_SEED, 0))[0]
    tin = torch.tensor([taus[0] / T])
    hk = _hip_kinks_split(m, x0[:, 0], tin, params, rows[0][0][0].reshape(-1), rows[0][0][1], N)
    run = lambda dt, kinks: FL.walk(FL.oracle_eps(_sd(), params, 0.0, T, taus, rows, dt, kinks=kinks, **KW), x0[:, 0], ab,   # noqa: E731
                                    taus, dt, [v] * S, npos=1)["q"][0]
    q64h = run(torch.float64, lambda k, half: _half(hk, 0, N))
    cap = Kinks()
    q32 = run(torch.float32, lambda k, half: cap)
    q64r = run(torch.float64, lambda k, half: Kinks(cap.relu, cap.pool))
    e, er = _rel_l2(q_hip, q64h), _rel_l2(q32, q64r)
    print(f"[flow q {math}] q hip {q_hip.tolist()} fp64 {q64h.tolist()}: hip {e:.3e} ref32 {er:.3e} ratio "
          f"{e / (3 * er + 2e-6):.2f}")
    _parity.record("flow_position_q", math=math, q_hip=q_hip.tolist(), q_fp64=q64h.tolist(), hip=e, ref32=er,
                   ratio=e / (3 * er + 2e-6))
    assert e <= 3 * er + 2e-6, (math, e, er)


# ---------------------------------------------------------------------------------------------------------------
# 5. the whole log_likelihood
# ---------------------------------------------------------------------------------------------------------------
RP = 2          # probe runs
_LL = {}


def _ref_loglik(form):
    """The fp32 and fp64 restatements with the kernel's probes of the runs 0..RP-1 (keys: the restated
    _flow_ref.run_key(RUN_SEED, r)), stacked over the probe runs."""
    if form not in _LL:
        x0, params = _problem()
        rows = _rows_by_step(1)
        out = {}
        for dt in (torch.float32, torch.float64):
            runs = []
            for r in range(RP):
                vs = [_kernel_probe(H, S + 1 - k, S, 0, FL.run_key(RUN_SEED, r))[0] for k in range(1, S + 1)]
                runs.append(FL.walk(FL.oracle_eps(_sd(), params, 0.0, T, _taus(), rows, dt, **KW), x0[:, 0], _ab(), _taus(),
                                    dt, vs, form))
            out[dt] = {k: torch.stack([r[k].double() for r in runs]) for k in ("logp", "prior", "logdet", "q", "x")}
        _LL[form] = out
    return _LL[form]


@pytest.mark.parametrize("math", ["h3", "fp32"])
@pytest.mark.parametrize("form", ["logdet", "trace"])
def test_log_likelihood_vs_fp64(math, form):
    """S = 4, R = 2: logp, prior, logdet and trace_hist against the restatement in fp64 with the kernel's probes, within
    the bar taken on logdet, and each quantity within its own too; shapes and dtypes of the FlowResult; the mean, the
    standard error and bits per dimension follow from logp_probe."""
    import cdm_amd
    x0, params = _problem()
    ref = _ref_loglik(form)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    d = cdm_amd.DDPM(_model(math), T)
    torch.manual_seed(SEED)
    res = d.log_likelihood(x0, params, steps=S, n_probe=RP, form=form, seed=RUN_SEED)
    Dn = H * H
    assert tuple(res.logp.shape) == (N,) and tuple(res.logp_probe.shape) == (RP, N) and tuple(res.latent.shape) == (N, 1, H, H)
    assert tuple(res.trace_hist.shape) == (RP, S, N) and res.invalid.dtype == torch.bool and not bool(res.invalid.any())
    assert all(t.dtype == torch.float64 and not t.is_cuda for t in (res.logp, res.logp_probe, res.stderr, res.bpd,
                                                                     res.prior, res.logdet, res.trace_hist))
    assert res.latent.dtype == torch.float32 and res.taus == _taus()
    assert torch.allclose(res.logp, res.logp_probe.mean(0), rtol=1e-15)
    assert torch.allclose(res.stderr, res.logp_probe.std(0) / np.sqrt(RP), rtol=1e-12)
    assert torch.allclose(res.bpd, -res.logp / (Dn * np.log(2.0)), rtol=1e-15)
    assert torch.allclose(res.logp, res.prior + res.logdet, rtol=1e-12)
    fig = {}
    for name, got, k in (("logdet", res.logdet, "logdet"), ("logp", res.logp, "logp"), ("prior", res.prior, "prior")):
        want64, want32 = r64[k].mean(0), r32[k].mean(0)
        fig[name] = (_rel_l2(got, want64), _rel_l2(want32, want64))
    fig["trace_hist"] = (_rel_l2(res.trace_hist, r64["q"]), _rel_l2(r32["q"], r64["q"]))
    fig["latent"] = (_rel_l2(res.latent[:, 0], r64["x"][0]), _rel_l2(r32["x"][0], r64["x"][0]))
    ratio = {k: e / (3 * er + 2e-6) for k, (e, er) in fig.items()}
    print(f"[flow loglik {math} {form}] logp {res.logp.tolist()} fp64 {r64['logp'].mean(0).tolist()} stderr "
          f"{res.stderr.tolist()}; (hip, ref32) {fig}; ratios {ratio}")
    _parity.record("flow_log_likelihood", math=math, form=form, logp=res.logp.tolist(), logp_fp64=r64["logp"].mean(0).tolist(),
                   stderr=res.stderr.tolist(), figures={k: dict(hip=e, ref32=er, ratio=ratio[k]) for k, (e, er) in fig.items()})
    bar = 3 * fig["logdet"][1] + 2e-6
    for k, (e, er) in fig.items():
        assert e <= 3 * er + 2e-6, (math, form, k, e, er)
        if k != "latent":
            assert e <= bar, (math, form, k, e, bar)


@pytest.mark.parametrize("math", ["fp32", "h3"])
def test_log_likelihood_determinism(math):
    """Two rows holding the same map and parameters give equal bits; the same seed gives the same bits across two calls and
    another seed other probes, none of them shared with the first seed's (seeds s and s ^ 1, runs 0 and 1), on the same
    sampler; R = 1 gives a NaN standard error; max_rows = 1 gives the unchunked bits (asserted under
    fp32, recorded under h3)."""
    import cdm_amd
    x0, params = _problem(n=3)
    x0[2], params[2] = x0[0], params[0]
    d = cdm_amd.DDPM(_model(math), T)
    call = lambda **kw: (torch.manual_seed(SEED), d.log_likelihood(x0, params, steps=S, **{**dict(seed=RUN_SEED), **kw}))[1]   # noqa: E731
    a, b, c = call(), call(), call(seed=RUN_SEED ^ 1)
    two, two_c = call(n_probe=2), call(seed=RUN_SEED ^ 1, n_probe=2)
    assert _bits(two.trace_hist[0], a.trace_hist[0]) and _bits(two_c.trace_hist[0], c.trace_hist[0])
    assert not any(_bits(two.trace_hist[i], two_c.trace_hist[j]) for i in range(2) for j in range(2))
    assert _bits(a.logp[0], a.logp[2]) and _bits(a.trace_hist[:, :, 0], a.trace_hist[:, :, 2]) and not _bits(a.logp[0], a.logp[1])
    assert all(_bits(getattr(a, k), getattr(b, k)) for k in ("logp", "logp_probe", "latent", "prior", "logdet", "trace_hist"))
    assert not _bits(a.trace_hist, c.trace_hist) and _bits(a.latent, c.latent)
    assert bool(torch.isnan(a.stderr).all())
    one = call(max_rows=1)
    same = all(_bits(getattr(a, k), getattr(one, k)) for k in ("logp", "latent", "prior", "trace_hist"))
    _parity.record("flow_chunking", math=math, max_rows_1_bit_identical=same,
                   logp_diff=float((a.logp - one.logp).abs().max()))
    print(f"[flow chunking {math}] max_rows=1 bit-identical: {same}")
    if math == "fp32":
        assert same
    assert sum(1 for k in d._samplers if k[0] == "flow") == 2          # one sampler per chunk size, whatever the seed


def test_log_likelihood_graph_replay_equals_eager():
    import cdm_amd
    m = _model("fp32")
    x0, params = _problem()
    d = cdm_amd.DDPM(m, T)
    out = []
    for kw in (dict(steps_per_graph=2), dict(use_graph=False)):
        smp = cdm_amd.FlowLikelihood(m, d.sched, N, params, steps=S, seed=RUN_SEED, **kw)
        torch.manual_seed(SEED)
        smp.prepare_rng(host_z=False)
        out.append(smp.run(x0, 2))
        assert (smp.graph is not None) == ("steps_per_graph" in kw)
    assert all(_bits(out[0][k], out[1][k]) for k in ("logp", "prior", "acc", "hist", "latent", "invalid"))


def test_api_errors_before_allocation():
    import cdm_amd
    x0, params = _problem()
    d = cdm_amd.DDPM(_model("fp32"), T)
    torch.manual_seed(1)
    state = torch.get_rng_state()
    for kw in (dict(guide_w=2.0), dict(form="exact"), dict(n_probe=0), dict(max_rows=0), dict(steps=T + 1), dict(seed=-1),
               dict(maps=x0[:, :, :8]), dict(params=params[:1])):
        with pytest.raises(ValueError):
            d.log_likelihood(**{**dict(maps=x0, params=params, steps=S), **kw})
    for kw in (dict(steps=T + 1), dict(maps=x0[:, :, :8]), dict(params=params[:, :5]), dict(guide_w=float("nan"))):
        with pytest.raises(ValueError):
            d.encode(**{**dict(maps=x0, params=params, steps=S), **kw})
    with pytest.raises(ValueError):
        cdm_amd.FlowLikelihood(_model("fp32"), d.sched, N, params, steps=S, guide_w=1.0)
    assert torch.equal(torch.get_rng_state(), state) and not d._samplers       # nothing drawn, nothing built
    m3 = cdm_amd.ContextUnet(3, NF, NCF, H).cuda().eval()
    d3 = cdm_amd.DDPM(m3, T)
    for fn in ("encode", "log_likelihood"):
        with pytest.raises(ValueError, match="in_channels"):
            getattr(d3, fn)(x0, params, steps=S)
    assert not d3._samplers
    r = cdm_amd.log_likelihood(_model("fp32"), x0[:, 0], None, T, steps=S)      # functional, no params, no channel axis
    assert tuple(r.logp.shape) == (N,) and bool(torch.isfinite(r.logp).all())
    xT = cdm_amd.encode(_model("fp32"), x0, T, params, steps=S)[0]
    assert tuple(xT.shape) == (N, 1, H, H) and bool(torch.isfinite(xT).all())


# ---------------------------------------------------------------------------------------------------------------
# 6. the round trip: recorded, not asserted
# ---------------------------------------------------------------------------------------------------------------
def test_round_trip_is_recorded():
    """sample_ddim_from_noise(encode(x), eta=0) over the same timesteps, beside the fp64 restatement's own round-trip
    error (same shortcut draws both ways there).  On untrained weights this shows nothing about quality: recorded only."""
    import cdm_amd
    x0, params = _problem()
    d = cdm_amd.DDPM(_model("fp32"), T, z_source="host")
    torch.manual_seed(SEED)
    xT, _ = d.encode(x0, params, steps=S)
    torch.manual_seed(SEED)
    back, _ = d.sample_ddim_from_noise(xT, params, steps=S, eta=0.0)
    rows = _rows_by_step(1)
    taus = _taus()
    x64 = _ref_encode(0.0)[1]
    cx, ce, _ = D.coefficients(_ab(), taus, 0.0, torch.float64)
    eps_fn = FL.oracle_eps(_sd(), params, 0.0, T, taus, rows[::-1], torch.float64, **KW)   # decoding draws in p = S..1 order
    x = x64
    with torch.no_grad():
        for p in range(S, 0, -1):
            x = cx[p] * x + ce[p] * eps_fn(x, p)
    e_hip, e_ref = _rel_l2(back, x0), _rel_l2(x, x0[:, 0])
    print(f"[flow round trip] hip {e_hip:.3e} fp64 restatement {e_ref:.3e}")
    _parity.record("flow_round_trip", hip=e_hip, fp64_restatement=e_ref)
    assert bool(torch.isfinite(back).all())
