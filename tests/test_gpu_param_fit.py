"""Parameter fit (cdm_amd.param_fit, likelihood.ParamFit) on the GPU: its three kernels alone (bit for bit against numpy
where the arithmetic is plain IEEE), and the fit against the torch-CPU restatement of its definition (tests/_fit_ref.py).

Network-level bar (the bar of tests/test_gpu_input_grads.py and test_gpu_param_scan.py): the relative L2 error of a
quantity against the fp64 restatement is at most 3x the fp32 restatement's own deviation from fp64, plus 2e-6.  For the
gradient both sides run on their own branch of the piecewise-linear network: HIP's ReLU / MaxPool decisions (read from
an engine forward per position, tests/_kinks.py) are imposed on the fp64 run HIP is compared with, the fp32
restatement's on the fp64 run it is compared with.

Model: the scan test's — n_feat 16, n_cfeat 6, H 64, eval mode, randomised BatchNorm running statistics; T = 20,
t_grid = [1, 10, 20], n_noise = 2 (P = 6 positions), M = 2 maps, a noise table passed as noise=; K = 2 starts, the
constant vectors 0.25 and 0.75.

Trajectory constants (chosen on the CPU, in the fp64 restatement alone): lr = 0.08, iters = 3 — every row's score falls
at each of the 3 iterations (by about 4e-7 of the score per iteration: the weights are untrained, so the context moves
the output little) and the smallest free gradient component is >= 5e-3 of the row's largest; 0.25 - 3 * 0.08 > 0, so
the default bounds never bind."""
import numpy as np
import pytest
import torch

import _fit_ref as FR
import _parity
import _scan_ref as SR
from _kinks import Kinks, hip_kinks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


NF, NCF, H, T = 16, 6, 64, 20
T_GRID, R_NOISE, M = [1, T // 2, T], 2, 2
P = len(T_GRID) * R_NOISE
START = torch.tensor([0.25, 0.75])[:, None].repeat(1, NCF)             # [K = 2, ncf]
SC_SEED = 31
ITERS, LR = 3, 0.08
KW = dict(n_feat=NF, n_cfeat=NCF, height=H)


def _rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _bits(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def _stream():
    return torch.cuda.current_stream().cuda_stream


p_ = lambda v: v.data_ptr()   # noqa: E731


# ------------------------------------------------------------------------------------------------------------------
# 1.-3. the kernels alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mk,K,HW", [(2, 3, 100), (1, 1, 4096), (3, 2, 4101)])
def test_fit_mse_grad_vs_numpy(Mk, K, HW):
    """cdm_fit_mse_grad: the accumulated score terms against numpy to relative 1e-12 (fp64 sums of <= 4101 terms differ
    by order at most near 4101 * 2^-53), with a column offset k0 = 2 in a wider accumulator (the other columns keep
    their bits) and two accumulating calls; deps bit for bit against coef * d in fp32 with coef = fp32((2 w inv_R) / HW)
    formed in fp64; a cur_i outside 1..T leaves acc and deps untouched; two runs give identical bits.  HW = 4101 puts
    rows off the 16-byte grid (scalar head, unaligned noise rows, scalar tail); HW = 100 keeps every row on it."""
    from cdm_amd._lib import lib
    g = torch.Generator().manual_seed(HW + 7 * K)
    pred, z = torch.randn(Mk * K, HW, generator=g), torch.randn(Mk, HW, generator=g)
    w = torch.rand(T + 1, generator=g) * 50 + 0.5
    k0, ld, inv_R = 2, K + 3, 1.0 / 3.0
    init = torch.randn(Mk, ld, generator=g, dtype=torch.float64)
    d = (pred.numpy().reshape(Mk, K, HW) - z.numpy()[:, None]).astype(np.float32)
    ssum = (d.astype(np.float64) ** 2).sum(-1)
    wi = lambda i: np.float64(w[i].item())                                        # noqa: E731
    term = lambda i: ((wi(i) * ssum) / HW) * inv_R                                # noqa: E731
    coef = lambda i: np.float32(((2.0 * wi(i)) * inv_R) / HW)                     # noqa: E731
    want = init.numpy().copy()
    want[:, k0:k0 + K] += term(3)
    want[:, k0:k0 + K] += term(T)
    pd, zd, wd = pred.cuda(), z.cuda(), w.cuda()
    runs = []
    for _ in range(2):
        acc = init.cuda()
        deps = torch.full((Mk * K, HW), 7.0, device="cuda")
        for i in (0, T + 1, -2):                                                   # write nothing
            cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
            lib().cdm_fit_mse_grad(p_(pd), p_(zd), Mk, K, HW, p_(cur), p_(wd), T, inv_R, p_(acc), ld, k0, p_(deps),
                                   _stream())
        assert _bits(acc, init) and bool((deps == 7.0).all())
        seen = []
        for i in (3, T):
            cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
            lib().cdm_fit_mse_grad(p_(pd), p_(zd), Mk, K, HW, p_(cur), p_(wd), T, inv_R, p_(acc), ld, k0, p_(deps),
                                   _stream())
            seen.append(deps.cpu().clone())
            assert _bits(seen[-1], torch.from_numpy((coef(i) * d).astype(np.float32).reshape(Mk * K, HW))), i
        runs.append((acc.cpu(), seen))
    got = runs[0][0].numpy()
    rel = np.abs(got[:, k0:k0 + K] - want[:, k0:k0 + K]) / np.abs(want[:, k0:k0 + K] - init.numpy()[:, k0:k0 + K])
    print(f"fit_mse_grad ({Mk},{K},{HW}): max rel err of the accumulated terms {rel.max():.3e}")
    assert rel.max() <= 1e-12
    keep = [c for c in range(ld) if not k0 <= c < k0 + K]
    assert _bits(runs[0][0][:, keep], init[:, keep])
    assert _bits(runs[0][0], runs[1][0]) and all(_bits(a, b) for a, b in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize("off_pred,off_noise,off_deps", [(1, 0, 1), (0, 3, 0), (0, 0, 1), (2, 1, 3)])
def test_fit_mse_grad_misaligned_buffers(off_pred, off_noise, off_deps):
    """Buffers that start off the 16-byte grid (views offset by 1..3 floats), HW = 203, M = 2, K = 2: pred and deps with
    the same offset (scalar head, float4 body), an unaligned noise (its float4 read falls back to scalars), and pred /
    deps that disagree mod 16 (the whole row scalar).  deps bit for bit, the score term to 1e-12, and the floats
    around deps keep their bits."""
    from cdm_amd._lib import lib
    Mk, K, HW, i = 2, 2, 203, 5
    g = torch.Generator().manual_seed(off_pred + 4 * off_noise + 16 * off_deps)
    pred, z = torch.randn(Mk * K, HW, generator=g), torch.randn(Mk, HW, generator=g)
    w = torch.rand(T + 1, generator=g) + 0.5
    pbuf, zbuf = torch.zeros(Mk * K * HW + 8, device="cuda"), torch.zeros(Mk * HW + 8, device="cuda")
    dbuf = torch.full((Mk * K * HW + 8,), 7.0, device="cuda")
    pv, zv = pbuf[off_pred:off_pred + Mk * K * HW], zbuf[off_noise:off_noise + Mk * HW]
    dv = dbuf[off_deps:off_deps + Mk * K * HW]
    pv.copy_(pred.reshape(-1)); zv.copy_(z.reshape(-1))
    assert pv.data_ptr() % 16 == 4 * off_pred and dv.data_ptr() % 16 == 4 * off_deps
    acc = torch.zeros(Mk, K, dtype=torch.float64, device="cuda")
    cur = torch.full((1,), i, dtype=torch.int32, device="cuda")
    wd = w.cuda()
    lib().cdm_fit_mse_grad(p_(pv), p_(zv), Mk, K, HW, p_(cur), p_(wd), T, 0.5, p_(acc), K, 0, p_(dv), _stream())
    d = (pred.numpy().reshape(Mk, K, HW) - z.numpy()[:, None]).astype(np.float32)
    wi = np.float64(w[i].item())
    coef = np.float32(((2.0 * wi) * 0.5) / HW)
    assert _bits(dv.cpu().reshape(Mk * K, HW), torch.from_numpy((coef * d).astype(np.float32).reshape(Mk * K, HW)))
    assert bool((dbuf[:off_deps] == 7.0).all()) and bool((dbuf[off_deps + Mk * K * HW:] == 7.0).all())
    want = ((wi * (d.astype(np.float64) ** 2).sum(-1)) / HW) * 0.5
    assert (np.abs(acc.cpu().numpy() - want) / want).max() <= 1e-12


@pytest.mark.parametrize("rows", [1, 7, 256])
def test_fit_grad_accum_bits(rows):
    from cdm_amd._lib import lib
    g = torch.Generator().manual_seed(rows)
    want = torch.randn(rows, NCF, generator=g, dtype=torch.float64)
    acc = want.cuda()
    for _ in range(3):
        dc = torch.randn(rows, NCF, generator=g) * 1e-3
        lib().cdm_fit_grad_accum(p_(dc.cuda()), rows, NCF, p_(acc), _stream())
        want = want + dc.double()
    assert _bits(acc, want)


@pytest.mark.parametrize("rows", [1, 5, 256])
def test_fit_update_bits(rows):
    """cdm_fit_update over 3 iterations, the closing pass and one call past it, against the numpy fp64 restatement bit
    for bit (plain IEEE fp64 with contraction off: equality is the derivable bar): c64, c32, m, v, best, history,
    stalled, the counter.  Gradients include an exact 0, values that push past each bound (lr 0.7 > hi - lo), a NaN row
    and an inf-score row; columns 1 and 4 are not free.  The call also clears score and gacc and resets the position
    counter; past the closing pass it changes nothing."""
    from cdm_amd._lib import lib
    g = np.random.default_rng(100 + rows)
    iters = 3
    free = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    lo, hi = np.full(NCF, 0.2), np.linspace(0.7, 0.8, NCF)
    lr, b1, b2, eps = 0.7, 0.9, 0.999, 1e-8
    c0 = g.uniform(0.2, 0.7, (rows, NCF)).astype(np.float32)
    st = FR.new_state(c0, iters)
    bc = FR.bias_table(b1, b2, iters)
    D = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).cuda() if dt is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()                   # noqa: E731
    dev = dict(c64=D(st["c64"]), c32=D(st["c32"]), m=D(st["m"]), v=D(st["v"]), best_score=D(st["best_score"]),
               best_c=D(st["best_c"]), hist_score=D(st["hist_score"]), hist_gnorm=D(st["hist_gnorm"]),
               stalled=D(st["stalled"]))
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    pos = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    mask_d, lo_d, hi_d, bc_d = D(free), D(lo), D(hi), D(bc)

    def same():
        for k, v in dev.items():
            a, b = v.cpu().numpy(), np.ascontiguousarray(st[k])
            if k == "hist_gnorm":                      # a NaN's payload is not part of the contract
                nan = np.isnan(b)
                assert (np.isnan(a) == nan).all(), k
                a, b = np.where(nan, 0.0, a), np.where(nan, 0.0, b)
            assert a.tobytes() == b.tobytes(), k
    for n in range(iters + 2):
        score = g.uniform(1, 2, rows)
        grad = g.standard_normal((rows, NCF)) * 1e-3
        grad[0, 0] = 0.0
        if n == 1:
            grad[min(1, rows - 1), 2] = np.nan
        if n == 2:
            score[rows - 1] = np.inf
        if n == 0:
            score[:] = np.sort(score)[::-1] + 3                                    # later passes find better scores
        sd_, gd_ = D(score), D(grad)
        pos.fill_(5)
        lib().cdm_fit_update(p_(done), iters, rows, NCF, p_(sd_), p_(gd_), p_(mask_d), p_(lo_d), p_(hi_d), lr, b1, b2,
                             eps, p_(bc_d), p_(dev["c64"]), p_(dev["c32"]), p_(dev["m"]), p_(dev["v"]),
                             p_(dev["best_score"]), p_(dev["best_c"]), p_(dev["hist_score"]), p_(dev["hist_gnorm"]),
                             p_(dev["stalled"]), p_(pos), _stream())
        FR.update(st, score, grad, iters, free, lo, hi, lr, b1, b2, eps, bc)
        same()
        assert done.item() == st["done"] == min(n + 1, iters + 1)
        if n <= iters:
            assert not sd_.any() and not gd_.any() and pos.item() == 0
        else:                                                                      # past the closing pass: untouched
            assert _bits(sd_, torch.from_numpy(score)) and _bits(gd_, torch.from_numpy(grad)) and pos.item() == 5
    assert st["stalled"].sum() == 2
    if rows > 1:
        assert (st["c64"][:, free == 1] == 0.2).any() and (st["c64"][:, free == 1] == hi[free == 1]).any()


# ------------------------------------------------------------------------------------------------------------------
# 4.-7. the fit on a model
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
    return _state_dict(), x, noise, SR.draw_rows(SC_SEED, P, NF)


@pytest.fixture(scope="module")
def trajectory(inputs):
    """The restatement's whole fit (iters 3, lr 0.08, both starts, both maps) in fp32 and fp64: computed once."""
    sd, x, noise, rows = inputs
    start = START[None].expand(M, -1, -1).contiguous()
    return {dt: FR.fit(sd, x, start, T, T_GRID, R_NOISE, noise, rows, dt, ITERS, LR, **KW)
            for dt in (torch.float32, torch.float64)}


_MODELS = {}


def _model(math, sd):
    import cdm_amd
    if math not in _MODELS:
        m = cdm_amd.ContextUnet(1, NF, NCF, H, conv_math=math)
        m.load_state_dict(sd)
        _MODELS[math] = m.cuda().eval()
    return _MODELS[math]


def _positions(x, noise):
    """(t, x_p [M,1,H,H], t / T) per position, as the restatement forms them."""
    from oracle import ref_cpu as R
    _, _, ab_t = R.make_schedule(T)
    sab, omab = ab_t.sqrt(), 1 - ab_t
    out = []
    for p in range(P):
        t = T_GRID[p % len(T_GRID)]
        out.append((t, (sab[t] * x + omab[t] * noise[p])[:, None], torch.tensor([t / T])))
    return out


def _hip_kinks_chunked(m, xp, tin, c, sc, kc):
    """HIP's decisions for the rows m K + k of c [Mx, K, ncf], read from one engine forward per chunk of kc starts (the
    batches the fit runs: under h3 the operand scale is taken over the chunk's batch) and put back in row order."""
    Mx, K = c.shape[:2]
    parts = []
    for k0 in range(0, K, kc):
        cc = c[:, k0:k0 + kc]
        n = cc.shape[1]
        relu, pool = hip_kinks(m, xp.repeat_interleave(n, 0), tin, cc.reshape(Mx * n, NCF), sc, frozen=True)
        idx = (torch.arange(Mx)[:, None] * K + k0 + torch.arange(n)[None]).reshape(-1)
        parts.append((idx, relu, pool))
    if len(parts) == 1:
        return parts[0][1], parts[0][2]

    def gather(items):
        out = torch.empty((Mx * K,) + tuple(items[0][1].shape[1:]), dtype=items[0][1].dtype)
        for idx, v in items:
            out[idx] = v
        return out
    relu = [(gather([(i, r[j][0]) for i, r, _ in parts]), gather([(i, r[j][1]) for i, r, _ in parts]))
            for j in range(len(parts[0][1]))]
    pool = [gather([(i, q[j]) for i, _, q in parts]) for j in range(len(parts[0][2]))]
    return relu, pool


def _grad_bar(tag, m, g_hip, sd, x, noise, rows, c, kc=None):
    """g_hip [Mx, K, ncf] against fp64 autograd of the restatement on HIP's branch (read from forwards of kc starts per
    batch, default all K); the fp32 restatement against fp64 on its own branch; HIP within 3x + 2e-6.  Prints and
    records before it asserts."""
    Mx, K = c.shape[:2]
    pos = _positions(x, noise)
    hk = []
    for (t, xp, tin), sc in zip(pos, rows):
        hk.append(_hip_kinks_chunked(m, xp, tin, c, sc, kc or K))
    ev = lambda dt, kinks: FR.evaluate(sd, x, c, T, T_GRID, R_NOISE, noise, rows, dt, kinks=kinks, **KW)   # noqa: E731
    s64h, g64h = ev(torch.float64, lambda p: Kinks(*hk[p]))
    cap32 = [Kinks() for _ in range(P)]
    s32, g32 = ev(torch.float32, lambda p: cap32[p])
    s64r, g64r = ev(torch.float64, lambda p: Kinks(cap32[p].relu, cap32[p].pool))
    eh, er = _rel_l2(g_hip, g64h), _rel_l2(g32, g64r)
    print(f"[{tag}] g: hip {eh:.3e} ref32 {er:.3e} ratio {eh / (3 * er + 2e-6):.2f}")
    _parity.record("param_fit_grad", tag=tag, hip=eh, ref32=er, ratio=eh / (3 * er + 2e-6))
    assert eh <= 3 * er + 2e-6, (tag, eh, er)
    return s64h, s32, s64r


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_gradient_vs_oracle(math, inputs):
    """One evaluation's g [M, K, ncf] at the two starts against the fp64 restatement on HIP's branch (_grad_bar)."""
    from cdm_amd import ParamFit
    sd, x, noise, rows = inputs
    m = _model(math, sd)
    pf = ParamFit(m, T, use_graph=False)
    torch.manual_seed(SC_SEED)
    score, g = pf.value_and_grad(x, START, t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
    assert g.shape == (M, 2, NCF) and g.dtype == torch.float64 and score.shape == (M, 2)
    c = START[None].expand(M, -1, -1).contiguous()
    s64h, s32, s64r = _grad_bar(f"grad/{math}", m, g, sd, x, noise, rows, c)
    assert _rel_l2(score, s64h) <= 3 * _rel_l2(s32, s64r) + 2e-6


def test_gradient_one_row(inputs):
    """M Kc = 1: the one-row c path of the embedding backward, within the bar."""
    from cdm_amd import ParamFit
    sd, x, noise, rows = inputs
    m = _model("fp32", sd)
    pf = ParamFit(m, T, use_graph=False)
    torch.manual_seed(SC_SEED)
    _, g1 = pf.value_and_grad(x[:1], START[:1], t_grid=T_GRID, n_noise=R_NOISE, noise=noise[:, :1])
    _grad_bar("grad/fp32/one_row", m, g1, sd, x[:1], noise[:, :1], rows, START[:1][None].contiguous())


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_chunked_vs_unchunked(math, inputs, trajectory):
    """max_rows = M (Kc = 1: two chunks of one start) against one chunk of both starts.  The chunked gradient meets the
    bar against the restatement on the branch of its own per-chunk forwards, under both arithmetics.  On the fp32
    arithmetic every kernel computes a batch row independently of the batch, so the chunked gradient and the whole
    chunked fit (params, score, histories, stalled) equal the unchunked bits; under h3 the operand scale is taken over
    the chunk's batch, so there the chunked fit is held to the bar of the history and its difference to the unchunked
    one is recorded."""
    import cdm_amd
    from cdm_amd import ParamFit
    sd, x, noise, rows = inputs
    m = _model(math, sd)
    pf = ParamFit(m, T, use_graph=False)
    c = START[None].expand(M, -1, -1).contiguous()
    kw = dict(t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
    out = []
    for max_rows in (256, M):
        torch.manual_seed(SC_SEED)
        out.append(pf.value_and_grad(x, START, max_rows=max_rows, **kw))
    assert len(pf._runs) == 2                                      # the (M, 2) run and the (M, 1) run
    _grad_bar(f"grad/{math}/chunked", m, out[1][1], sd, x, noise, rows, c, kc=1)
    fits = []
    for max_rows in (256, M):
        torch.manual_seed(SC_SEED)
        fits.append(cdm_amd.param_fit(m, x, START, T, iters=ITERS, lr=LR, max_rows=max_rows, **kw))
    h64 = trajectory[torch.float64]["hist_score"]
    hist = fits[1].history_score.cpu().numpy().reshape(ITERS + 1, -1)
    eh, er = _rel_l2(hist, h64), _rel_l2(trajectory[torch.float32]["hist_score"], h64)
    same = _bits(out[0][1], out[1][1]) and _bits(out[0][0], out[1][0]) and _all_bits(fits[0], fits[1])
    dp = (fits[0].last_params - fits[1].last_params).abs().max().item()
    print(f"[chunk/{math}] history: hip {eh:.3e} ref32 {er:.3e}; bit-identical to unchunked: {same}; g rel diff "
          f"{_rel_l2(out[1][1], out[0][1]):.3e}, |last_params diff| {dp:.3e}")
    _parity.record("param_fit_chunking", math=math, bit_identical=same, g_rel_diff=_rel_l2(out[1][1], out[0][1]),
                   last_params_diff=dp, history=dict(hip=eh, ref32=er))
    assert eh <= 3 * er + 2e-6 and (np.diff(hist, axis=0) < 0).all()
    assert _bits(fits[1].score, fits[1].history_score.min(0).values)
    assert _bits(fits[1].start, fits[0].start) and not fits[1].stalled.any()
    if math == "fp32":
        assert same


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_stop_after_gives_the_full_backwards_dc(math, inputs):
    """backward(stop_after="up0emb") writes the same dc bits as the full backward after the same forward on the same
    workspace (the skipped stages come after dc), and leaves the encoder's gradients unwritten."""
    sd, x, noise, rows = inputs
    m = _model(math, sd)
    eng, Pm = m._engine_and_params()
    s = _stream()
    eng.repack(Pm, True, s)
    eng.train_pack_token = object()
    m._invalidate_eval_pack()
    B = 3
    g = torch.Generator().manual_seed(2)
    xin = torch.rand(B, H, H, generator=g).cuda()
    t, c = torch.tensor([0.4]).cuda(), torch.rand(B, NCF, generator=g).cuda()
    deps = torch.randn(B, H, H, generator=g).cuda()
    scw, scb = (v.reshape(-1).cuda() for v in rows[0])
    ws = eng.workspace(B, True, frozen=True)
    out = []
    for stop in (None, "up0emb"):
        G = {n: torch.full_like(Pm[n], 9.0) for n in m._param_names}
        dc = torch.zeros(B, NCF, device="cuda")
        eng.forward(ws, Pm, xin, t, c, scw, scb, B, s, frozen=True)
        eng.backward(ws, Pm, deps, G, s, dc=dc, stop_after=stop)
        torch.cuda.synchronize()
        out.append((dc.clone(), G))
    assert out[0][0].abs().max() > 0 and _bits(out[0][0], out[1][0])
    assert _bits(out[0][1]["up1.model.0.weight"], out[1][1]["up1.model.0.weight"])
    assert bool((out[1][1]["down1.model.0.conv1.0.weight"] == 9.0).all())
    assert not bool((out[0][1]["down1.model.0.conv1.0.weight"] == 9.0).all())
    with pytest.raises(AssertionError):
        eng.backward(ws, Pm, deps, out[0][1], s, stop_after="down2")


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_trajectory(math, inputs, trajectory):
    """iters = 3 from both starts: the restatement's preconditions (checked here, on the CPU values), then the GPU's
    history falls likewise and meets the bar against the fp64 history; |params - restatement| is measured, recorded and
    held to 10x the fp32 restatement's own deviation from fp64.
    Measured (profiles/param_fit_parity.jsonl): |last_params - fp64| 2.0e-5 under h3 and 3.4e-3 under fp32, the fp32
    restatement's own 3.4e-3 - so at these inputs the 10x bar (3.4e-2) is loose.  The cause, found on the CPU: at the
    start the fp32 restatement takes one ReLU decision of row (map 0, start 0.25) differently from fp64; on that row its
    gradient is 1e-3 off instead of 1e-6, and column 1, the row's smallest component (6e-3 of its largest), is 13 % off.
    Adam normalises every component, so that one column lands 3.4e-3 away after three steps; every other entry of the
    fp32 restatement is within 1.5e-5, and the rows without a flip within 4.2e-7.  On the GPU the fp32 arithmetic lands
    1.8e-5 from the fp32 restatement (3.4e-3 from fp64) and h3 2.0e-5 from fp64 (3.4e-3 from the fp32 restatement): each
    sits beside one of the two CPU runs, as a shared decision would have it.  Which branch an arithmetic takes at a
    decision inside its rounding error is chance, so no bar for the direct difference can be derived: it is recorded
    (params_vs_ref32), and the bar stays the issue's.  The tight checks are the history bar here and the gradient on
    HIP's own branch in test_gradient_vs_oracle."""
    import cdm_amd
    sd, x, noise, rows = inputs
    r32, r64 = trajectory[torch.float32], trajectory[torch.float64]
    h64 = r64["hist_score"]
    assert (np.diff(h64, axis=0) < 0).all(), h64
    for gg in r64["g"][:ITERS]:
        a = np.abs(gg).reshape(-1, NCF)
        assert (a.min(1) >= 1e-3 * a.max(1)).all()
    m = _model(math, sd)
    torch.manual_seed(SC_SEED)
    res = cdm_amd.param_fit(m, x, START, T, iters=ITERS, lr=LR, t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
    hist = res.history_score.cpu().numpy().reshape(ITERS + 1, -1)
    assert res.history_score.shape == (ITERS + 1, M, 2) and res.params.shape == (M, 2, NCF)
    assert res.params.dtype == torch.float32 and res.score.dtype == torch.float64
    eh, er = _rel_l2(hist, h64), _rel_l2(r32["hist_score"], h64)
    dev32 = np.abs(r32["c32"].astype(np.float64) - r64["c32"]).max()
    got = np.abs(res.last_params.cpu().numpy().reshape(-1, NCF).astype(np.float64) - r64["c32"]).max()
    gotb = np.abs(res.params.cpu().numpy().reshape(-1, NCF).astype(np.float64) - r64["best_c"]).max()
    gn = _rel_l2(res.history_grad_norm.reshape(ITERS + 1, -1), r64["hist_gnorm"])
    direct = np.abs(res.last_params.cpu().numpy().reshape(-1, NCF).astype(np.float64) - r32["c32"]).max()
    print(f"[traj/{math}] history: hip {eh:.3e} ref32 {er:.3e}; falls {(np.diff(hist, axis=0) < 0).all()}; "
          f"|last_params - fp64| {got:.3e}, |params - fp64| {gotb:.3e}, ref32 {dev32:.3e}; gnorm rel {gn:.3e}")
    _parity.record("param_fit_trajectory", math=math, history=dict(hip=eh, ref32=er), falls=bool((np.diff(hist, axis=0) < 0).all()),
                   last_params_abs=got, params_abs=gotb, ref32_params_abs=dev32, params_vs_ref32=direct, grad_norm_rel=gn,
                   drop_per_iter=(-np.diff(h64, axis=0)).min() / h64.max())
    assert (np.diff(hist, axis=0) < 0).all(), hist
    assert eh <= 3 * er + 2e-6
    bar = 10 * dev32
    assert got <= bar and gotb <= bar, (got, gotb, bar)
    assert _bits(res.score, res.history_score.min(0).values) and _bits(res.start_score, res.history_score[0])
    assert not res.stalled.any() and res.stalled.dtype == torch.int32
    assert torch.equal(res.best(), res.params[torch.arange(M), res.score.argmin(1).cpu()].to(res.params.device))
    if math == "h3":                                            # DDPM.param_fit is the same call
        torch.manual_seed(SC_SEED)
        short = cdm_amd.DDPM(m, T).param_fit(x, START, iters=ITERS, lr=LR, t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
        assert _bits(short.params, res.params) and _bits(short.history_score, res.history_score)


def test_free_columns_and_bounds(inputs):
    """free = [0, 3]: the other four columns of params and last_params are the start's bits.  Bounds the first step
    (size lr = 0.08) would leave: the result lies inside them, on a bound where the step pushed out."""
    import cdm_amd
    sd, x, noise, _ = inputs
    m = _model("h3", sd)
    kw = dict(iters=ITERS, lr=LR, t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
    torch.manual_seed(SC_SEED)
    res = cdm_amd.param_fit(m, x, START, T, free=[0, 3], **kw)
    start = START[None].expand(M, -1, -1).cuda()
    keep = [1, 2, 4, 5]
    assert _bits(res.params[..., keep], start[..., keep]) and _bits(res.last_params[..., keep], start[..., keep])
    assert (res.last_params[..., [0, 3]] != start[..., [0, 3]]).all()
    torch.manual_seed(SC_SEED)
    tight = cdm_amd.param_fit(m, x, START[:1], T, bounds=(0.22, 0.28), **kw)
    for v in (tight.params, tight.last_params):
        assert (v >= np.float32(0.22)).all() and (v <= np.float32(0.28)).all()
    assert ((tight.last_params == np.float32(0.22)) | (tight.last_params == np.float32(0.28))).any()


def _all_bits(a, b):
    return all(_bits(getattr(a, k), getattr(b, k)) for k in
               ("params", "score", "last_params", "history_score", "history_grad_norm", "stalled"))


def test_graph_equals_eager_and_device_noise(inputs):
    """steps_per_graph = 2 over P = 6 positions (three replays per pass) equals the eager loop bit for bit, as does
    steps_per_graph = 8 > P (nothing captured); two identical calls give identical bits.  Device Philox noise
    (noise=None): K = 1 gives the same bits as column 0 of a K = 2 fit on the fp32 arithmetic (rows do not interact)."""
    from cdm_amd import ParamFit
    sd, x, noise, _ = inputs
    m = _model("h3", sd)
    kw = dict(iters=2, lr=LR, t_grid=T_GRID, n_noise=R_NOISE)

    def run(pf, start=START, **extra):
        torch.manual_seed(SC_SEED)
        return pf.fit(x, start, **kw, **extra)
    g2, g8, eager = ParamFit(m, T, steps_per_graph=2), ParamFit(m, T, steps_per_graph=8), ParamFit(m, T, use_graph=False)
    a = run(g2, noise=noise)
    assert next(iter(g2._runs.values())).graph is not None
    b = run(g8, noise=noise)
    assert next(iter(g8._runs.values())).graph is None
    assert _all_bits(a, run(eager, noise=noise)) and _all_bits(a, b) and _all_bits(a, run(g2, noise=noise))
    d2 = run(g2, seed=77)
    assert _all_bits(d2, run(eager, seed=77)) and not _bits(d2.history_score, a.history_score)
    mf = _model("fp32", sd)
    f2 = ParamFit(mf, T, steps_per_graph=2)
    k2, k1 = run(f2, seed=77), run(f2, START[:1], seed=77)
    assert _bits(k1.history_score[..., 0], k2.history_score[..., 0]) and _bits(k1.params[:, 0], k2.params[:, 0])


@pytest.mark.parametrize("math", ["h3", "fp32"])
def test_consistent_with_scan(math, inputs, trajectory):
    """param_scan at the start vectors and history_score[0] of a fit after the same torch.manual_seed see the same
    objective through differently structured forwards (folded eval pack vs frozen train-structured): each within the
    bar against the shared restatement; the direct difference is measured and recorded."""
    import cdm_amd
    sd, x, noise, _ = inputs
    m = _model(math, sd)
    kw = dict(t_grid=T_GRID, n_noise=R_NOISE, noise=noise)
    torch.manual_seed(SC_SEED)
    scan = cdm_amd.param_scan(m, x, START, T, **kw).score
    torch.manual_seed(SC_SEED)
    fit0 = cdm_amd.param_fit(m, x, START, T, iters=1, lr=LR, **kw).start_score
    s32 = trajectory[torch.float32]["hist_score"][0].reshape(M, 2)
    s64 = trajectory[torch.float64]["hist_score"][0].reshape(M, 2)
    er = _rel_l2(s32, s64)
    es, ef, direct = _rel_l2(scan, s64), _rel_l2(fit0, s64), _rel_l2(fit0, scan)
    print(f"[scan_vs_fit/{math}] scan {es:.3e} fit {ef:.3e} ref32 {er:.3e}; fit vs scan {direct:.3e}")
    _parity.record("param_fit_vs_scan", math=math, scan=es, fit=ef, ref32=er, direct=direct)
    assert es <= 3 * er + 2e-6 and ef <= 3 * er + 2e-6
    top = cdm_amd.ScanResult(scan, START, T_GRID).top(2)
    assert top.shape == (M, 2, NCF)
