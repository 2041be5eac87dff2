"""Observation-guided sampling (diffusion posterior sampling on the captured step graph): the two kernels bit for bit
against tests/_guided_ref.py, their argument checks, the total image gradient and a whole trajectory against the fp64
restatement on the oracle's forward, the zeta = 0 form against the plain DDIM sampler, graph replay, reuse, determinism,
the pack hand-over to other users of the engine, and the public interface.

Model: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64) in eval mode with randomised BatchNorm running
statistics; T = 100, S = 4, n = 2.  The bar of every comparison with fp64 is the project's: relative L2 <= 3 x the fp32
restatement's own deviation from fp64 + 2e-6; every figure is printed and recorded before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
import _guided_ref as GR
import _parity
from _kinks import Kinks, first_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NF, NCF, H, N, T, S = 8, 6, 64, 2, 100, 4
KW = dict(n_feat=NF, n_cfeat=NCF, height=H)
INVALID = 1          # hipErrorInvalidValue
SEED = 77


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sd():
    fx = np.load(os.path.join(GOLD, "model_nf8.npz"))
    sd = {k[3:]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith("sd.")}
    g = torch.Generator().manual_seed(11)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    return sd


_MODELS = {}


def _model(math="fp32"):
    import cdm_amd
    if math not in _MODELS:
        m = cdm_amd.ContextUnet(1, NF, NCF, H, conv_math=math)
        m.load_state_dict(_sd())
        _MODELS[math] = m.cuda().eval()
    return _MODELS[math]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def _rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _i32(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).cuda()


def _taus():
    return D.subsequence(T, S)


def _ab():
    return R.make_schedule(T)[2]


def _problem(seed=3, f=4, n=N):
    """x_T, params, an observation of random maps with noise, and weights with holes (one plane for the batch)."""
    import cdm_amd
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, 1, H, H, generator=g)
    params = torch.rand(n, NCF, generator=g)
    obs = cdm_amd.degrade(torch.rand(n, 1, H, H, generator=g), f, sigma=0.05, seed=seed + 1)
    wgt = 0.5 + torch.rand(1, 1, H // f, H // f, generator=g)
    wgt[..., :3, :] = 0
    wgt[..., 5, 7] = 0
    return x_T, params, obs, wgt


def _draws(seed, eta, sets, n=N):
    """The CPU-RNG draws of one run after torch.manual_seed(seed), in the sampler's order: per position z (eta > 0 and
    p > 1), then the shortcut draw(s).  -> (rows[S - p] = [(w, b)] * sets, zs[S - p])."""
    torch.manual_seed(seed)
    rows, zs = [], []
    for p in range(S, 0, -1):
        zs.append(torch.randn(n, 1, H, H)[:, 0] if eta > 0 and p > 1 else None)
        rows.append([R.draw_shortcut(1, NF) for _ in range(sets)])
    return rows, zs


# ---------------------------------------------------------------------------------------------------------------
# 1. cdm_obs_residual_grad, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [8, 64])
@pytest.mark.parametrize("f", [1, 2, 4, 8])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("per_sample", [False, True])
def test_obs_residual_grad_kernel_bit_exact(f, h, cfg, per_sample):
    """deps, gdir, L and the hist row = tests/_guided_ref.residual_grad in fp32 (L: the kernel's summation order restated,
    so exact bits are asked for, not 1 ulp), n = 3, at two positions.  The weight plane has zero cells whose obs is NaN
    (never read); with a per-sample weight, sample 1 is all zero: L = 0 exactly.  The null-output (zeta = 0) form writes
    the same L.  Two runs give the same bits."""
    from cdm_amd._lib import lib
    lb = lib()
    n, npos, w = 3, 5, 1.75
    hc = h // f
    g = torch.Generator().manual_seed(100 * f + h + cfg)
    x, ec, eu = (torch.randn(n, h, h, generator=g) for _ in range(3))
    obs = torch.randn(n, hc, hc, generator=g)
    wgt = torch.rand(n if per_sample else 1, hc, hc, generator=g) + 0.1
    wgt[0, 0, 0] = 0
    wgt[0, hc // 2, : hc // 2 + 1] = 0
    if per_sample:
        wgt[1] = 0
    obs[(wgt == 0).expand(n, hc, hc)] = float("nan")
    sq = torch.rand(npos + 1, generator=g); ra = 1 + torch.rand(npos + 1, generator=g)
    B = 2 * n if cfg else n
    eps = torch.cat([ec, eu]) if cfg else ec
    d = lambda t: t.contiguous().cuda()    # noqa: E731
    xd, ed, od, wd, sqd, rad = d(x), d(eps), d(obs), d(wgt), d(sq), d(ra)
    for p in (2, npos):
        cur = _i32([p])
        want = GR.residual_grad(x, ec, eu if cfg else None, w, obs, wgt, f, sq[p], ra[p])
        outs = []
        for rep in range(2):
            L = torch.full((n,), -1.0, dtype=torch.float64).cuda()
            hist = torch.full((npos + 1, n), -1.0, dtype=torch.float64).cuda()
            deps, gdir = torch.full((B, h, h), 9.0).cuda(), torch.full((n, h, h), 9.0).cuda()
            lb.cdm_obs_residual_grad(_ptr(xd), _ptr(ed), int(cfg), w, _ptr(od), _ptr(wd), wd.numel(), n, h, f,
                                     _ptr(cur), _ptr(sqd), _ptr(rad), npos, _ptr(L), _ptr(hist), _ptr(deps), _ptr(gdir),
                                     _stream())
            torch.cuda.synchronize()
            outs.append((L.cpu(), hist.cpu(), deps.cpu(), gdir.cpu()))
        L, hist, deps, gdir = outs[0]
        assert all(_bits(a, b) for a, b in zip(outs[0], outs[1])), "two runs differ"
        assert _bits(gdir, want["gdir"]), (f, h, cfg, p)
        assert _bits(deps[:n], want["deps_c"])
        if cfg:
            assert _bits(deps[n:], want["deps_u"])
        exact = _bits(L, want["L"])
        ulp = float(((L - want["L"]).abs() / torch.from_numpy(np.spacing(want["L"].numpy())).clamp_min(1e-300)).max())
        _parity.record("guided_residual_L", f=f, h=h, cfg=cfg, per_sample=per_sample, p=p, exact=exact, ulp=ulp)
        assert exact, (L, want["L"], ulp)
        assert _bits(hist[p], L) and bool((hist[[q for q in range(npos + 1) if q != p]] == -1).all())
        if per_sample:
            assert L[1].item() == 0.0 and bool((gdir[1] == 0).all()) and bool((deps[1] == 0).all())
        assert bool(torch.isfinite(deps).all()) and bool(torch.isfinite(gdir).all())
        # the zeta == 0 form: L only
        L0 = torch.full((n,), -1.0, dtype=torch.float64).cuda()
        hist0 = torch.full((npos + 1, n), -1.0, dtype=torch.float64).cuda()
        lb.cdm_obs_residual_grad(_ptr(xd), _ptr(ed), int(cfg), w, _ptr(od), _ptr(wd), wd.numel(), n, h, f, _ptr(cur),
                                 _ptr(sqd), _ptr(rad), npos, _ptr(L0), _ptr(hist0), None, None, _stream())
        assert _bits(L0.cpu(), L) and _bits(hist0.cpu(), hist)


# ---------------------------------------------------------------------------------------------------------------
# 2. cdm_ddim_step_guided, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.6])
def test_ddim_step_guided_kernel_bit_exact(cfg, eta):
    """x, both halves of the model-input buffer and the snapshot slot = tests/_guided_ref.guided_update in fp32 at every
    position of a 5-position walk (host z table), n = 3 with an L == 0 sample, whose x has the DDIM step's bits; zeta = 0
    (null gradient inputs) equals cdm_ddim_step_pos bit for bit; a position out of range writes nothing."""
    from cdm_amd._lib import lib
    from cdm_amd.diffusion import ddim_tables, snapshot_slots
    lb = lib()
    n, h, npos, w, zeta = 3, 20, 5, 1.5, 0.8
    numel = n * h * h
    taus = D.subsequence(T, npos)
    cx, ce, sg = (torch.from_numpy(v) for v in ddim_tables(_ab(), taus, eta))
    slots, nslots = snapshot_slots(npos, 2)
    g = torch.Generator().manual_seed(17 + cfg)
    x, ec, eu, gd, dxc, dxu = (torch.randn(n, h, h, generator=g) for _ in range(6))
    ztab = torch.randn(npos - 1, n, h, h, generator=g)
    L = torch.tensor([2.5, 0.0, 0.3], dtype=torch.float64)
    B = 2 * n if cfg else n
    d = lambda t: t.contiguous().cuda()    # noqa: E731
    eps_d = d(torch.cat([ec, eu]) if cfg else ec)
    dx_d = d(torch.cat([dxc, dxu]) if cfg else dxc)
    gd_d, L_d, z_d, cxd, ced, sgd, slot_d = d(gd), d(L), d(ztab), d(cx), d(ce), d(sg), _i32(slots)

    def launch(p, zt, guided=True, pos=False):
        xbuf = d(torch.cat([x, x]) if cfg else x)
        snaps = torch.full((nslots, numel), 7.0).cuda()
        cur = _i32([p])
        args = (_ptr(xbuf), _ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(eps_d), int(cfg), w, _ptr(cur), _ptr(cxd),
                _ptr(ced), _ptr(sgd), npos, _ptr(z_d), numel, 1234, None, _ptr(slot_d), _ptr(snaps))
        if pos:
            lb.cdm_ddim_step_pos(*args, _stream())
        elif guided:
            lb.cdm_ddim_step_guided(*args, _ptr(gd_d), _ptr(dx_d), _ptr(L_d), zt, h, _stream())
        else:
            lb.cdm_ddim_step_guided(*args, None, None, None, 0.0, h, _stream())
        torch.cuda.synchronize()
        return xbuf.cpu(), snaps.cpu()

    for p in range(npos, 0, -1):
        z = ztab[npos - p] if p > 1 else None
        want = GR.guided_update(x, ec, eu if cfg else None, w, cx[p], ce[p], sg[p], z, gd, dxc, dxu if cfg else None, L,
                                zeta)
        plain = D.step(x, ec, eu if cfg else None, torch.tensor(w), cx[p], ce[p], sg[p], z)
        xb, snaps = launch(p, zeta)
        assert _bits(xb[:n], want), (cfg, eta, p)
        if cfg:
            assert _bits(xb[n:], want)
        assert _bits(xb[1], plain[1]) and not _bits(xb[0], plain[0])            # the L == 0 sample: the DDIM step
        if slots[p] >= 0:
            assert _bits(snaps[slots[p]].reshape(n, h, h), want)
        assert bool((snaps[[q for q in range(nslots) if q != slots[p]]] == 7.0).all())
        x0, s0 = launch(p, 0.0, guided=False)
        xp, sp = launch(p, 0.0, pos=True)
        assert _bits(x0, xp) and _bits(s0, sp) and _bits(x0[:n], plain)
    for p in (0, npos + 1, -3):
        xb, snaps = launch(p, zeta)
        assert _bits(xb[:n], x) and bool((snaps == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# 3. hipErrorInvalidValue
# ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing():
    from cdm_amd._lib import lib
    lb = lib()
    n, h, f, npos = 2, 8, 2, 3
    cells = (h // f) ** 2
    numel = n * h * h
    F32 = lambda *sh: torch.full(sh, 5.0).cuda()    # noqa: E731
    x, eps, obs, wgt, sq, ra = F32(n, h, h), F32(2 * n, h, h), F32(n * cells), F32(cells), F32(npos + 1), F32(npos + 1)
    L, hist = torch.full((n,), 5.0, dtype=torch.float64).cuda(), torch.full((npos + 1, n), 5.0, dtype=torch.float64).cuda()
    deps, gdir = F32(2 * n, h, h), F32(n, h, h)
    cur = _i32([2])
    good = dict(x=_ptr(x), eps=_ptr(eps), cfg=0, w=0.0, obs=_ptr(obs), wgt=_ptr(wgt), wgt_numel=cells, n=n, H=h, f=f,
                cur_k=_ptr(cur), sq=_ptr(sq), ra=_ptr(ra), npos=npos, L=_ptr(L), hist=_ptr(hist), deps=_ptr(deps),
                gdir=_ptr(gdir), stream=_stream())
    raw = lb.raw("cdm_obs_residual_grad")
    bad = [dict(x=None), dict(eps=None), dict(obs=None), dict(wgt=None), dict(cur_k=None), dict(sq=None), dict(ra=None),
           dict(L=None), dict(hist=None), dict(f=3), dict(f=0), dict(f=16), dict(H=9), dict(wgt_numel=cells + 1),
           dict(wgt_numel=3 * cells), dict(deps=None), dict(gdir=None), dict(n=0), dict(npos=0)]
    for kw in bad:
        assert raw(*{**good, **kw}.values()) == INVALID, kw
    raw2 = lb.raw("cdm_ddim_step_guided")
    cx = F32(npos + 1)
    dx, Ld = F32(2 * n, h, h), torch.ones(n, dtype=torch.float64).cuda()
    xb, snaps, slot = F32(n, h, h), F32(2, numel), _i32([0, 0, 1, -1])
    good2 = dict(xin=_ptr(xb), x=_ptr(xb), x2=None, numel=numel, eps=_ptr(eps), cfg=0, w=0.0, cur_k=_ptr(cur), cx=_ptr(cx),
                 ce=_ptr(cx), sigma=_ptr(cx), npos=npos, z_table=None, zstride=numel, seed=1, seed_dev=None,
                 snap_slot=_ptr(slot), snaps=_ptr(snaps), grad_dir=_ptr(gdir), dx=_ptr(dx), L=_ptr(Ld), zeta=0.5, H=h,
                 stream=_stream())
    bad2 = [dict(xin=None), dict(x=None), dict(eps=None), dict(cur_k=None), dict(cx=None), dict(ce=None), dict(sigma=None),
            dict(npos=0), dict(numel=0), dict(zstride=-1), dict(snaps=None), dict(H=0), dict(H=5), dict(zeta=-0.5),
            dict(zeta=float("nan")), dict(zeta=float("inf")), dict(grad_dir=None), dict(dx=None), dict(L=None)]
    for kw in bad2:
        assert raw2(*{**good2, **kw}.values()) == INVALID, kw
    torch.cuda.synchronize()
    for t in (L, hist, deps, gdir, xb, snaps):
        assert bool((t == 5.0).all())


# ---------------------------------------------------------------------------------------------------------------
# 4.-5. the total gradient of one position and a trajectory against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------
def _hip_kinks_split(m, x, t, c, sc_w, sc_b, split):
    """tests/_kinks.hip_kinks for a batch whose halves take two shortcut draws (CFG: ``split`` = n < B): HIP's ReLU /
    MaxPool decisions in the oracle's call order, read from one frozen engine forward of all B rows."""
    eng, P = m._engine_and_params()
    B = x.shape[0]
    s = _stream()
    eng.repack(P, True, s)
    eng.train_pack_token = object()
    m._invalidate_eval_pack()
    ws = eng.workspace(B, True, frozen=True)
    eng.forward(ws, P, x.cuda().reshape(B, H, H), t.cuda(), c.cuda(), sc_w.cuda(), sc_b.cuda(), split, s, frozen=True)
    torch.cuda.synchronize()

    def z_of(y, scale, shift, C, Sz, per_sample):
        y = y.double().cpu().reshape(B, Sz, Sz, C)
        sc_ = scale.double().cpu().reshape(B if per_sample else 1, 1, 1, C)
        sh = shift.double().cpu().reshape(B if per_sample else 1, 1, 1, C)
        return (y * sc_ + sh).float().permute(0, 3, 1, 2).contiguous()

    relu, pool = [], []
    for i, l in enumerate(eng.layers):
        st = ws.bn[l.name]
        z = z_of(ws.y[l.name], st["scale"], st["shift"], l.cout, l.S, False)
        relu.append((z > 0, z))
        if l.name in ("down1.model.1.conv2", "down2.model.1.conv2"):
            Bz, C, Sz, _ = z.shape
            r = torch.relu(z)
            win = r.reshape(Bz, C, Sz // 2, 2, Sz // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bz, C, Sz // 2, Sz // 2, 4)
            pool.append(first_max(win))
        if i == 9:
            z0 = z_of(ws.y0, ws.gn0["scale"], ws.gn0["shift"], 2 * NF, H // 4, True)
            relu.append((z0 > 0, z0))
    zO = z_of(ws.yO, ws.gnO["scale"], ws.gnO["shift"], NF, H, True)
    relu.append((zO > 0, zO))
    return relu, pool


def _half(k, lo, hi):
    relu, pool = k
    return Kinks([(a[lo:hi], b[lo:hi]) for a, b in relu], [q[lo:hi] for q in pool])


@pytest.mark.parametrize("math", ["h3", "fp32"])
@pytest.mark.parametrize("w", [0.0, 2.0])
def test_one_position_gradient_vs_fp64(math, w):
    """grad = gdir + dx (+ the uncond rows' dx) of the first position (p = S) against fp64 autograd of the restatement on
    HIP's own ReLU / MaxPool branch; the fp32 restatement against fp64 on its own branch gives the bar."""
    import cdm_amd
    m = _model(math)
    x_T, params, obs, wgt = _problem()
    taus, ab, zeta = _taus(), _ab(), 0.5
    cfg = w > 0
    sets = 2 if cfg else 1
    rows, zs = _draws(SEED, 0.0, sets)
    d = cdm_amd.DDPM(m, T, z_source="host")
    smp = cdm_amd.GuidedDDIMSampler(m, d.sched, N, w, params, steps=S, z_source="host", use_graph=False, factor=4,
                                    weight_n=1, zeta=zeta)
    torch.manual_seed(SEED)
    smp.prepare_rng(host_z=True)
    smp.run(x_T, steps=1, obs=obs, weight=wgt)
    torch.cuda.synchronize()
    grad = smp.gdir.cpu() + smp.dx[:N].cpu() + (smp.dx[N:].cpu() if cfg else 0)
    L_hip = smp.hist[S].cpu()
    # HIP's branch, from one forward of the batch the sampler ran
    tin = torch.tensor([taus[-1] / T])
    xin = x_T[:, 0].repeat(sets, 1, 1)
    cc = torch.cat([params, torch.zeros_like(params)]) if cfg else params
    sc_w = torch.cat([r[0].reshape(-1) for r in rows[0]]); sc_b = torch.cat([r[1] for r in rows[0]])
    hk = _hip_kinks_split(m, xin, tin, cc, sc_w, sc_b, N)
    sd = _sd()
    run = lambda dt, kinks: GR.trajectory(sd, x_T[:, 0], params, w, T, ab, taus, 0.0, obs[:, 0], wgt[:, 0], 4, zeta,   # noqa: E731
                                          rows, zs, dt, kinks=kinks, keep=True, npos=1, **KW)[2][0]
    r64h = run(torch.float64, lambda p, half: _half(hk, half * N, (half + 1) * N))
    cap = [Kinks(), Kinks()]
    r32 = run(torch.float32, lambda p, half: cap[half])
    r64r = run(torch.float64, lambda p, half: Kinks(cap[half].relu, cap[half].pool))
    eh, er = _rel_l2(grad, r64h["grad"]), _rel_l2(r32["grad"], r64r["grad"])
    lh, lr = _rel_l2(L_hip, r64h["L"]), _rel_l2(r32["L"], r64r["L"])
    print(f"[guided grad {math} w={w}] grad: hip {eh:.3e} ref32 {er:.3e} ratio {eh / (3 * er + 2e-6):.2f}; "
          f"L: hip {lh:.3e} ref32 {lr:.3e}")
    _parity.record("guided_position_grad", math=math, w=w, hip=eh, ref32=er, ratio=eh / (3 * er + 2e-6), L_hip=lh,
                   L_ref32=lr)
    assert eh <= 3 * er + 2e-6, (math, w, eh, er)
    assert lh <= 3 * lr + 2e-6, (math, w, lh, lr)


_TRAJ = {}


def _ref_trajectory(eta, zeta, w=0.0):
    """The fp32 and fp64 restatement trajectories of the shared problem, computed once per (eta, zeta, w)."""
    key = (eta, zeta, w)
    if key not in _TRAJ:
        x_T, params, obs, wgt = _problem()
        rows, zs = _draws(SEED, eta, 2 if w > 0 else 1)
        out = {}
        caps = {}
        for dt in (torch.float32, torch.float64):
            caps[dt] = {}

            def kinks(p, half, dt=dt):
                caps[dt][(p, half)] = Kinks()
                return caps[dt][(p, half)]
            out[dt] = GR.trajectory(_sd(), x_T[:, 0], params, w, T, _ab(), _taus(), eta, obs[:, 0], wgt[:, 0], 4, zeta,
                                    rows, zs, dt, kinks=kinks, **KW)
        flips = sum(int((a[0] != b[0]).sum()) for k in caps[torch.float32]
                    for a, b in zip(caps[torch.float32][k].relu, caps[torch.float64][k].relu))
        _TRAJ[key] = (out[torch.float32], out[torch.float64], flips)
    return _TRAJ[key]


@pytest.mark.parametrize("math", ["h3", "fp32"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_trajectory_vs_fp64(math, eta):
    """Four positions, f = 4, weights with holes, zeta = 0.5, host z: x and the misfit history against the free-running
    fp64 restatement; the fp32 restatement's deviation gives the bar.  The number of ReLU decisions in which the fp32
    restatement leaves the fp64 branch is counted and recorded (each is a kink of the gradient, not of x)."""
    import cdm_amd
    x_T, params, obs, wgt = _problem()
    zeta = 0.5
    (x32, m32), (x64, m64), flips = _ref_trajectory(eta, zeta)
    d = cdm_amd.DDPM(_model(math), T, z_source="host")
    torch.manual_seed(SEED)
    x, inter, misfit = d.reconstruct(obs, params, 0.0, factor=4, weight=wgt, zeta=zeta, steps=S, eta=eta, noise=x_T)
    assert tuple(x.shape) == (N, 1, H, H) and tuple(misfit.shape) == (S + 1, N) and misfit.dtype == torch.float64
    ex, er = _rel_l2(x[:, 0], x64), _rel_l2(x32, x64)
    em, emr = _rel_l2(misfit, m64), _rel_l2(m32, m64)
    print(f"[guided trajectory {math} eta={eta}] x: hip {ex:.3e} ref32 {er:.3e} ratio {ex / (3 * er + 2e-6):.2f}; misfit: "
          f"hip {em:.3e} ref32 {emr:.3e}; fp32-vs-fp64 ReLU flips {flips}; misfit first/last "
          f"{misfit[0].tolist()} / {misfit[-1].tolist()}")
    _parity.record("guided_trajectory", math=math, eta=eta, x=dict(hip=ex, ref32=er, ratio=ex / (3 * er + 2e-6)),
                   misfit=dict(hip=em, ref32=emr, ratio=em / (3 * emr + 2e-6)), relu_flips_ref32_vs_fp64=flips,
                   misfit_first=misfit[0].tolist(), misfit_last=misfit[-1].tolist())
    assert ex <= 3 * er + 2e-6, (math, eta, ex, er)
    assert em <= 3 * emr + 2e-6, (math, eta, em, emr)


# ---------------------------------------------------------------------------------------------------------------
# 6. zeta = 0 is the plain DDIM sampler
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, 2.0])
def test_zeta_zero_vs_sample_ddim(w):
    """reconstruct(zeta=0) and sample_ddim_from_noise on the same x_T and shortcut draws, both within the bar of the
    fp64 restatement of the plain walk; whether the frozen forward and the eval forward give the same bits is recorded,
    not asserted.  The misfit history is still recorded, and the unguided final misfit is printed beside the guided one."""
    import cdm_amd
    x_T, params, obs, wgt = _problem()
    (x32, m32), (x64, m64), _ = _ref_trajectory(0.0, 0.0, w)
    d = cdm_amd.DDPM(_model("fp32"), T, z_source="host")
    torch.manual_seed(SEED)
    xg, _, misfit = d.reconstruct(obs, params, w, factor=4, weight=wgt, zeta=0.0, steps=S, noise=x_T)
    torch.manual_seed(SEED)
    xp, _ = d.sample_ddim_from_noise(x_T, params, steps=S, guide_w=w)
    er = _rel_l2(x32, x64)
    eg, ep = _rel_l2(xg[:, 0], x64), _rel_l2(xp[:, 0], x64)
    same = _bits(xg, xp)
    torch.manual_seed(SEED)
    _, _, guided = d.reconstruct(obs, params, w, factor=4, weight=wgt, zeta=0.5, steps=S, noise=x_T)
    print(f"[guided zeta=0 w={w}] guided sampler {eg:.3e} plain sampler {ep:.3e} ref32 {er:.3e}; bits equal: {same}; final "
          f"misfit unguided {misfit[-1].tolist()} guided (zeta 0.5) {guided[-1].tolist()}")
    _parity.record("guided_zeta0_vs_ddim", w=w, guided=eg, plain=ep, ref32=er, bit_identical=same,
                   misfit_unguided=misfit[-1].tolist(), misfit_guided=guided[-1].tolist())
    assert eg <= 3 * er + 2e-6 and ep <= 3 * er + 2e-6
    assert _rel_l2(misfit, m64) <= 3 * _rel_l2(m32, m64) + 2e-6
    assert smp_of(d, zeta=0.0).dx is None and smp_of(d, zeta=0.0).G is None      # nothing of the backward is allocated


def smp_of(d, **match):
    return next(s for k, s in d._samplers.items() if k[0] == "guided" and all(getattr(s, a) == v for a, v in match.items()))


# ---------------------------------------------------------------------------------------------------------------
# 7.-10. graph replay, reuse, determinism, the pack hand-over
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, 2.0])
def test_graph_replay_equals_eager(w):
    import cdm_amd
    m = _model("fp32")
    x_T, params, obs, wgt = _problem()
    d = cdm_amd.DDPM(m, T, z_source="host")
    out = []
    for kw in (dict(steps_per_graph=2), dict(use_graph=False)):
        smp = cdm_amd.GuidedDDIMSampler(m, d.sched, N, w, params, steps=S, eta=0.5, z_source="host", factor=4, weight_n=1,
                                        zeta=0.5, save_rate=2, **kw)
        torch.manual_seed(SEED)
        smp.prepare_rng(host_z=True)
        out.append(smp.run(x_T, obs=obs, weight=wgt))
        assert (smp.graph is not None) == ("steps_per_graph" in kw)
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][2], out[1][2])
    assert np.array_equal(out[0][1], out[1][1]) and out[0][1].shape[1:] == (N, 1, H, H)


def test_second_call_reuses_sampler_and_graph():
    import cdm_amd
    m = _model("fp32")
    x_T, params, obs, wgt = _problem()
    obs2, wgt2 = obs.flip(0) + 0.1, wgt.flip(-1)
    d = cdm_amd.DDPM(m, T, z_source="host")
    kw = dict(factor=4, zeta=0.5, steps=S, noise=x_T)
    torch.manual_seed(SEED)
    a = d.reconstruct(obs, params, weight=wgt, **kw)
    smp = smp_of(d)
    graph = smp.graph
    assert graph is not None or S < smp.K
    torch.manual_seed(SEED)
    b = d.reconstruct(obs2, params, weight=wgt2, **kw)
    assert len(d._samplers) == 1 and smp_of(d) is smp and smp.graph is graph
    torch.manual_seed(SEED)
    fresh = cdm_amd.DDPM(m, T, z_source="host").reconstruct(obs2, params, weight=wgt2, **kw)
    assert _bits(b[0], fresh[0]) and _bits(b[2], fresh[2]) and not _bits(a[0], b[0])


def test_device_noise_determinism():
    import cdm_amd
    x_T, params, obs, wgt = _problem()
    d = cdm_amd.DDPM(_model("fp32"), T, z_source="device")
    kw = dict(factor=4, weight=wgt, zeta=0.5, steps=S, eta=0.5, noise=x_T)
    out = []
    for cs in (5, 5, 6):
        torch.manual_seed(SEED); torch.cuda.manual_seed(cs)
        out.append(d.reconstruct(obs, params, **kw))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][2], out[1][2]) and not _bits(out[0][0], out[2][0])


def test_other_users_of_the_engine_after_a_reconstruct():
    """A plain sample_ddim and a Trainer.step on the same model give the results they give without a reconstruct in
    between: the guided sampler's train pack is not mistaken for theirs."""
    import cdm_amd
    from cdm_amd import Trainer
    x_T, params, obs, wgt = _problem()

    def fresh():
        m = cdm_amd.ContextUnet(1, NF, NCF, H)
        m.load_state_dict(_sd())
        return m.cuda().eval()

    def plain(d):
        torch.manual_seed(SEED)
        return d.sample_ddim_from_noise(x_T, params, steps=S)[0]

    g = torch.Generator().manual_seed(8)
    x0, c = torch.rand(N, 1, H, H, generator=g).cuda(), torch.rand(N, NCF, generator=g).cuda()
    inject = (torch.randn(N, 1, H, H, generator=g).cuda(), torch.tensor([7, 60], dtype=torch.int32).cuda(),
              torch.cat([v.reshape(-1) for v in R.draw_shortcut(1, NF)]).cuda())

    def train(m):
        tr = Trainer(m.train(), 1e-3, T, N, seed=3)
        loss = tr.step(x0, c, inject=inject).clone()
        torch.cuda.synchronize()
        return loss.cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    ma, mb = fresh(), fresh()
    da, db = cdm_amd.DDPM(ma, T, z_source="host"), cdm_amd.DDPM(mb, T, z_source="host")
    want_x = plain(da)
    first = plain(db)
    torch.manual_seed(SEED)
    db.reconstruct(obs, params, factor=4, weight=wgt, zeta=0.5, steps=S, noise=x_T)
    assert _bits(first, want_x) and _bits(plain(db), want_x)
    loss_a, sd_a = train(ma)
    torch.manual_seed(SEED)
    db.reconstruct(obs, params, factor=4, weight=wgt, zeta=0.5, steps=S, noise=x_T)
    loss_b, sd_b = train(mb)
    assert _bits(loss_a, loss_b) and all(_bits(sd_a[k], sd_b[k]) for k in sd_a)


# ---------------------------------------------------------------------------------------------------------------
# 11. the public interface
# ---------------------------------------------------------------------------------------------------------------
def test_api_shapes_and_errors():
    import cdm_amd
    x_T, params, obs, wgt = _problem()
    d = cdm_amd.DDPM(_model("fp32"), T)
    torch.manual_seed(1)
    state = torch.get_rng_state()
    for kw in (dict(sampler="ddpm"), dict(sampler="dpmpp"), dict(resample=2), dict(jump=2), dict(t_start=50),
               dict(known=x_T, mask=torch.ones(1, 1, H, H)), dict(factor=3), dict(zeta=-1.0), dict(weight=-wgt),
               dict(noise=x_T[:1]), dict(steps=T + 1), dict(eta=-1.0), dict(z_source="gpu")):
        with pytest.raises(ValueError):
            d.reconstruct(obs, params, **{**dict(steps=S, factor=4), **kw})
    with pytest.raises(ValueError):
        d.reconstruct(obs[:, :, :8], params, steps=S)
    assert torch.equal(torch.get_rng_state(), state) and not d._samplers       # nothing drawn, nothing built
    m3 = cdm_amd.ContextUnet(3, NF, NCF, H).cuda().eval()
    with pytest.raises(ValueError, match="in_channels"):
        cdm_amd.DDPM(m3, T).reconstruct(obs, params, steps=S)
    x, inter, misfit = d.reconstruct(obs[:, 0], None, steps=S, factor=4, save_rate=2)       # no params, no weight, drawn x_T
    assert tuple(x.shape) == (N, 1, H, H) and x.is_cuda and bool(torch.isfinite(x).all())
    assert inter.shape == (S, N, 1, H, H) and tuple(misfit.shape) == (S + 1, N) and not misfit.is_cuda
    assert np.array_equal(inter[-1], x.cpu().numpy()) and bool((misfit > 0).all())
    per = wgt.expand(N, -1, -1, -1).clone()
    d.reconstruct(obs, params, 2.0, factor=4, weight=per, steps=S, eta=0.3)
    assert len(d._samplers) == 2
    with pytest.raises(ValueError):
        cdm_amd.GuidedDDIMSampler(_model("fp32"), d.sched, N, 0.0, None, steps=S, factor=4, weight_n=3)
