"""Parameter scan (cdm_amd.param_scan, likelihood.ParamScan) on the GPU: its two kernels alone, and the scan against a
torch-CPU restatement of its definition on the oracle's forward (tests/_scan_ref.py).

Network-level bar (_bar; the bar of tests/test_gpu_input_grads.py): the relative L2 error of a quantity against the
fp64 restatement is at most 3x the fp32 restatement's own deviation from fp64 on the same quantity, plus 2e-6.  It is
held for the scores and for the differences score[:, k] - score[:, 0], which are the signal of a scan.

Model: n_feat 16, n_cfeat 6, H 64, eval mode, torch.manual_seed weights, randomised BatchNorm running statistics (the
same state under both conv arithmetics, so one reference serves both).  T = 20, t_grid = [1, 10, 20], n_noise = 2
(P = 6 positions), M = 2 maps, candidates = the constant vectors 0, 0.5, 1 (and 0.25 for the chunking test)."""
import numpy as np
import pytest
import torch

import _parity
import _scan_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


NF, NCF, H, T = 16, 6, 64, 20
T_GRID, R_NOISE, M = [1, T // 2, T], 2, 2
P = len(T_GRID) * R_NOISE
CAND = torch.tensor([0.0, 0.5, 1.0, 0.25])[:, None].repeat(1, NCF)
SC_SEED = 31


def _rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _bits(a, b):
    return torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 100), (1, 1, 4096), (3, 2, 4096)]


@pytest.mark.parametrize("Mk,K,HW", SHAPES)
def test_scan_perturb_equals_perturb_on_repeated_rows(Mk, K, HW):
    """cdm_scan_perturb == cdm_perturb on repeat_interleave'd inputs, bit for bit, at every timestep class (first, a
    middle one, last); a cur_i outside 1..T writes nothing."""
    from cdm_amd import Schedule
    from cdm_amd._lib import lib
    sched = Schedule(T, "cuda")
    g = torch.Generator().manual_seed(HW + K)
    x, z = torch.rand(Mk, HW, generator=g).cuda(), torch.randn(Mk, HW, generator=g).cuda()
    xr, zr = x.repeat_interleave(K, 0).contiguous(), z.repeat_interleave(K, 0).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    p = lambda v: v.data_ptr()   # noqa: E731
    for i in (1, 7, T):
        cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
        out = torch.full((Mk * K, HW), float("nan"), device="cuda")
        ref = torch.empty(Mk * K, HW, device="cuda")
        lib().cdm_scan_perturb(p(x), p(z), p(cur), p(sched.sab), p(sched.omab), Mk, K, HW, T, p(out), s)
        lib().cdm_perturb(p(xr), p(zr), None, p(cur), 0, p(sched.sab), p(sched.omab), Mk * K, HW, T, p(ref), None, s)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), i
    for i in (0, T + 1, -3):
        cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
        out = torch.full((Mk * K, HW), 7.0, device="cuda")
        lib().cdm_scan_perturb(p(x), p(z), p(cur), p(sched.sab), p(sched.omab), Mk, K, HW, T, p(out), s)
        assert (out == 7.0).all(), i


@pytest.mark.parametrize("Mk,K,HW", SHAPES)
def test_scan_mse_accum_vs_numpy_fp64(Mk, K, HW):
    """cdm_scan_mse_accum against its numpy restatement (d in fp32, squares and sum in fp64) to relative 1e-12 — fp64
    sums of <= 4096 terms differ by order at most near 4096 * 2^-53 = 4.5e-13 — with a column offset k0 = 2 inside a
    wider accumulator (the other columns keep their bits), two accumulating calls, cur_i outside 1..T leaving acc
    untouched, and two runs giving identical bits."""
    from cdm_amd._lib import lib
    g = torch.Generator().manual_seed(HW + 7 * K)
    pred, z = torch.randn(Mk * K, HW, generator=g), torch.randn(Mk, HW, generator=g)
    w = torch.rand(T + 1, generator=g) * 50 + 0.5
    k0, ld = 2, K + 3
    init = torch.randn(Mk, ld, generator=g, dtype=torch.float64)
    d = (pred.numpy().reshape(Mk, K, HW) - z.numpy()[:, None]).astype(np.float32)
    ssum = (d.astype(np.float64) ** 2).sum(-1)
    term = lambda i: (np.float64(w[i].item()) * ssum) / HW      # noqa: E731  (w[i].item(): the fp32 value, exactly)
    want = init.numpy().copy()
    want[:, k0:k0 + K] += term(3)
    want[:, k0:k0 + K] += term(T)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda v: v.data_ptr()   # noqa: E731
    pd, zd, wd = pred.cuda(), z.cuda(), w.cuda()
    runs = []
    for _ in range(2):
        acc = init.cuda()
        for i in (3, 0, T, T + 1):                                # 0 and T + 1 write nothing
            cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
            lib().cdm_scan_mse_accum(p(pd), p(zd), Mk, K, HW, p(cur), p(wd), T, p(acc), ld, k0, s)
        runs.append(acc.cpu())
    got = runs[0].numpy()
    rel = np.abs(got[:, k0:k0 + K] - want[:, k0:k0 + K]) / np.abs(want[:, k0:k0 + K] - init.numpy()[:, k0:k0 + K])
    print(f"scan_mse_accum ({Mk},{K},{HW}): max rel err of the accumulated terms {rel.max():.3e}")
    assert rel.max() <= 1e-12
    keep = [c for c in range(ld) if not k0 <= c < k0 + K]
    assert _bits(runs[0][:, keep], init[:, keep])
    assert _bits(runs[0], runs[1])


def test_scan_prologue_and_noise_row():
    """cdm_scan_prologue walks a position table with repeated timesteps and more positions than timesteps (what
    cdm_sample_prologue_sub's contract excludes); past the last position, or at a timestep outside 1..T, it sets
    cur_i = 0 and touches nothing else.  cdm_scan_noise_row copies row *cur_p of a table."""
    from cdm_amd._lib import lib
    Tn, pos = 3, [1, 3, 3, 2, 1, 9]                                # 6 positions > T = 3; position 5 is out of range
    dev = "cuda"
    I = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    ctr, cur_i, cur_p, pos_t = I(0), I(-1), I(-1), I(*pos)
    t_cur = torch.full((1,), -1.0, device=dev)
    table = torch.arange(6 * 5, dtype=torch.float32, device=dev).reshape(6, 5)
    sc_cur = torch.zeros(5, device=dev)
    ztab = torch.randn(6, 37, device=dev)
    zrow = torch.zeros(37, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda v: v.data_ptr()   # noqa: E731
    for k in range(5):
        lib().cdm_scan_prologue(p(ctr), 6, Tn, p(pos_t), p(cur_i), p(cur_p), p(t_cur), p(table), 5, p(sc_cur), s)
        lib().cdm_scan_noise_row(p(ztab), p(cur_p), 6, 37, p(zrow), s)
        assert (ctr.item(), cur_i.item(), cur_p.item()) == (k + 1, pos[k], k)
        assert t_cur.item() == np.float32(pos[k] / Tn)
        assert torch.equal(sc_cur, table[k]) and torch.equal(zrow, ztab[k])
    for _ in range(2):                                             # timestep 9 > T, then (ctr forced) past the end
        cur_i.fill_(2)
        lib().cdm_scan_prologue(p(ctr), 6, Tn, p(pos_t), p(cur_i), p(cur_p), p(t_cur), p(table), 5, p(sc_cur), s)
        assert cur_i.item() == 0 and cur_p.item() == 4 and torch.equal(sc_cur, table[4])
        ctr.fill_(6)


# ------------------------------------------------------------------------------------------------------------------
# 2.-6. the scan on a model
# ------------------------------------------------------------------------------------------------------------------
def _state_dict():
    import cdm_amd
    torch.manual_seed(3)
    m = cdm_amd.ContextUnet(1, NF, NCF, H)
    g = torch.Generator().manual_seed(17)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    return sd


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(23)
    x = torch.rand(M, H, H, generator=g)
    noise = torch.randn(P, M, H, H, generator=g)
    return _state_dict(), x, noise


@pytest.fixture(scope="module")
def reference(inputs):
    """Per-position MSEs of the restatement for the four candidates, fp32 and fp64: computed once, read-only."""
    sd, x, noise = inputs
    rows = SR.draw_rows(SC_SEED, P, NF)
    kw = dict(n_feat=NF, n_cfeat=NCF, height=H)
    return {dt: SR.position_mse(sd, x, CAND, T, T_GRID, R_NOISE, noise, rows, dt, **kw)
            for dt in (torch.float32, torch.float64)}


_MODELS = {}


def _model(math, sd):
    import cdm_amd
    if math not in _MODELS:
        m = cdm_amd.ContextUnet(1, NF, NCF, H, conv_math=math)
        m.load_state_dict(sd)
        _MODELS[math] = m.cuda().eval()
    return _MODELS[math]


def _bar(tag, got, reference, cols, weight):
    """The scores and their differences to candidate 0 against the fp64 restatement: each within 3x the fp32
    restatement's own error + 2e-6.  Prints and records every figure before it asserts."""
    r32, r64 = (SR.score(reference[dt][:, :, cols], T, T_GRID, R_NOISE, weight) for dt in (torch.float32, torch.float64))
    got = got.cpu()
    diff = lambda s: s[:, 1:] - s[:, :1]   # noqa: E731
    fig = {}
    for name, f in (("score", lambda s: s), ("diff", diff)):
        eh, er = _rel_l2(f(got), f(r64)), _rel_l2(f(r32), f(r64))
        fig[name] = dict(hip=eh, ref32=er, ratio=eh / (3 * er + 2e-6))
    print(f"[{tag}] " + ", ".join(f"{k}: hip {v['hip']:.3e} ref32 {v['ref32']:.3e} ratio {v['ratio']:.2f}"
                                  for k, v in fig.items()))
    _parity.record("param_scan_parity", tag=tag, **fig)
    for name, v in fig.items():
        assert v["hip"] <= 3 * v["ref32"] + 2e-6, (tag, name, v)


@pytest.mark.parametrize("weight", ["uniform", "nll"])
@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_scan_vs_oracle(math, weight, inputs, reference):
    """M = 2, K = 3, both weights, both conv arithmetics, the noise table and the shortcut rows of the restatement."""
    import cdm_amd
    sd, x, noise = inputs
    m = _model(math, sd)
    torch.manual_seed(SC_SEED)
    res = cdm_amd.param_scan(m, x, CAND[:3], T, t_grid=T_GRID, n_noise=R_NOISE, weight=weight, noise=noise)
    assert res.score.shape == (M, 3) and res.score.dtype == torch.float64 and res.score.is_cuda
    assert res.t_grid == T_GRID and torch.equal(res.candidates, CAND[:3])
    assert not m.training
    _bar(f"oracle/{math}/{weight}", res.score, reference, [0, 1, 2], weight)
    if weight == "uniform":                                     # DDPM.param_scan is the same call
        torch.manual_seed(SC_SEED)
        short = cdm_amd.DDPM(m, T).param_scan(x, CAND[:3], t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
        assert _bits(short.score, res.score)


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_scan_chunking(math, inputs, reference):
    """K = 4 in chunks of Kc = 2 (max_rows 4) and in one chunk of 4 (max_rows 8): both within the bar.  Whether the two
    are bit-identical is recorded, not asserted (h3 scales each operand by the maximum over the chunk's batch)."""
    import cdm_amd
    sd, x, noise = inputs
    m = _model(math, sd)
    out = []
    for max_rows in (4, 8):
        torch.manual_seed(SC_SEED)
        res = cdm_amd.param_scan(m, x, CAND, T, t_grid=T_GRID, n_noise=R_NOISE, noise=noise, max_rows=max_rows)
        _bar(f"chunk/{math}/Kc{max_rows // M}", res.score, reference, [0, 1, 2, 3], "uniform")
        out.append(res.score)
    same = _bits(out[0], out[1])
    print(f"[chunk/{math}] Kc = 2 and Kc = 4 bit-identical: {same}; rel diff {_rel_l2(out[0], out[1]):.3e}")
    _parity.record("param_scan_chunking", math=math, bit_identical=same, rel_diff=_rel_l2(out[0], out[1]))


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_scan_common_randomness(math, inputs):
    """Candidates [a, b, a]: columns 0 and 2 are the same bits (every eval kernel computes a batch row independently of
    its position; h3's operand scale is common to the tensor), and column 1 differs."""
    import cdm_amd
    sd, x, _ = inputs
    m = _model(math, sd)
    cand = CAND[[1, 2, 1]]
    torch.manual_seed(SC_SEED)
    s = cdm_amd.param_scan(m, x, cand, T, t_grid=T_GRID, n_noise=R_NOISE, seed=5).score
    assert torch.isfinite(s).all() and (s > 0).all()
    assert _bits(s[:, 0], s[:, 2])
    assert not torch.equal(s[:, 0], s[:, 1])


def test_scan_graph_equals_eager_and_seeds(inputs):
    """steps_per_graph = 2 over P = 6 positions (three replays) equals the eager loop bit for bit, as does a graph of 4
    (one replay + two eager steps); the same seed repeats the bits, another seed changes them."""
    from cdm_amd import ParamScan
    sd, x, _ = inputs
    m = _model("h3", sd)
    kw = dict(t_grid=T_GRID, n_noise=R_NOISE)

    def run(ps, seed):
        torch.manual_seed(SC_SEED)
        return ps.scan(x, CAND[:3], seed=seed, **kw).score.clone()
    g2, g4, eager = ParamScan(m, T, steps_per_graph=2), ParamScan(m, T, steps_per_graph=4), ParamScan(m, T, use_graph=False)
    a = run(g2, 11)
    assert next(iter(g2._runs.values())).graph is not None
    assert _bits(a, run(eager, 11)) and _bits(a, run(g4, 11))
    assert _bits(a, run(g2, 11))
    b = run(g2, 12)
    assert not torch.equal(a, b)
    assert _bits(b, run(eager, 12))


def test_scan_device_noise_is_philox_by_position(inputs):
    """noise=None draws z_p = cdm_philox_normal(seed, sub = p) over the M H W elements: that table fed back as noise=
    gives identical bits, also when the candidates are chunked (the noise does not depend on K or the chunking)."""
    import cdm_amd
    from cdm_amd._lib import lib
    sd, x, _ = inputs
    m = _model("h3", sd)
    seed = 987
    table = torch.empty(P, M, H, H, device="cuda")
    for p in range(P):
        lib().cdm_philox_normal(table[p].data_ptr(), M * H * H, seed, p, None, torch.cuda.current_stream().cuda_stream)
    kw = dict(t_grid=T_GRID, n_noise=R_NOISE)
    for max_rows in (256, 2):
        torch.manual_seed(SC_SEED)
        dev = cdm_amd.param_scan(m, x, CAND[:3], T, seed=seed, max_rows=max_rows, **kw).score
        torch.manual_seed(SC_SEED)
        tab = cdm_amd.param_scan(m, x, CAND[:3], T, noise=table, max_rows=max_rows, **kw).score
        assert _bits(dev, tab), max_rows
    torch.manual_seed(SC_SEED)
    host = cdm_amd.param_scan(m, x, CAND[:3], T, noise=table.cpu(), **kw).score      # a host table is the same table
    torch.manual_seed(SC_SEED)
    assert _bits(host, cdm_amd.param_scan(m, x, CAND[:3], T, seed=seed, **kw).score)
