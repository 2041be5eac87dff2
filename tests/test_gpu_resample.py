"""Position programs on the graph-captured strided samplers: RePaint resampling and late start (SDEdit).  The blend +
forward-jump kernel and the position-keyed DDIM step, their device noise, exact properties of a run, trajectory parity,
graph replay, reuse, determinism, public interface and CLI.  The definition is tests/_resample_ref.py (the reference has
neither).

Shapes: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64), n = 2, T = 100, S = 12 unless a test says otherwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
import _inpaint_ref as I
import _resample_ref as RS
import _parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
NF, NCF, H, N, T, S = 8, 6, 64, 2, 100, 12
INVALID = 1          # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sd():
    fx = np.load(os.path.join(GOLD, "model_nf8.npz"))
    return {k[3:]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith("sd.")}


@pytest.fixture(scope="module")
def model():
    import cdm_amd
    m = cdm_amd.ContextUnet(1, NF, NCF, H)
    m.load_state_dict(_sd())
    return m.cuda().eval()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _half_plane(n=1):
    m = torch.zeros(n, 1, H, H)
    m[..., : H // 2] = 1
    return m


def _known(seed=41, n=N):
    return torch.rand(n, 1, H, H, generator=torch.Generator().manual_seed(seed))


def _params(seed=31):
    return torch.rand(N, NCF, generator=torch.Generator().manual_seed(seed))


def _i32(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).cuda()


def _corr(u, v):
    u, v = u.double(), v.double()
    return float(((u - u.mean()) * (v - v.mean())).mean() / (u.std() * v.std()))


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    # cfg, mask ("full": per sample, "bcast": one for the batch, None: null mask), fresh, (n, h)
    (False, "full", False, (2, 64)),
    (True, "bcast", True, (2, 64)),
    (True, "full", False, (2, 64)),
    (False, "bcast", True, (2, 64)),
    (False, None, False, (2, 64)),
    (True, None, False, (2, 64)),
    (True, "full", True, (3, 20)),          # 1200 elements: the grid-stride tail (a last block partly filled)
    (False, "bcast", False, (3, 20)),
    (False, None, False, (3, 20)),
]


@pytest.mark.parametrize("cfg,mk,fresh,shape", KERNEL_CASES)
def test_mask_blend_jump_kernel_bit_exact(cfg, mk, fresh, shape):
    """cdm_mask_blend_jump = tests/_inpaint_ref.blend then tests/_resample_ref.forward_jump (separate fp32 torch-CPU ops on
    the same fp32 tables), bit for bit, at every position of the 11-position program of uniform(100, 7), J = 2, R = 2:
    jumping and non-jumping positions and the last (j = 0).  The state (and the second half of the model-input buffer
    under CFG) holds the jumped value, at known pixels too; the snapshot slot named for the position (and no other)
    holds the blended value before the jump.  xi is row P - p ("fresh") or 0 ("fixed"), zeta row P - p.  The mask is
    hard with a soft 0.25 band; ``known`` is NaN wherever its mask is 0, the xi table NaN at j = 0, the zeta table NaN at
    a position that does not jump (none of them read).  A position outside 1..P writes nothing."""
    import cdm_amd
    lb = cdm_amd.lib()
    n, h = shape
    ab_t = R.make_schedule(T)[2]
    taus = D.subsequence(T, 7)
    prog = cdm_amd.resample_program(ab_t, taus, jump=2, resamples=2)
    tr = RS.program(taus, 2, 2)
    Pn = prog.P
    assert Pn == 11 and len(tr) == 11
    sab, somab = (torch.from_numpy(v) for v in cdm_amd.known_tables(ab_t))
    fa, fb = torch.from_numpy(prog.fa), torch.from_numpy(prog.fb)
    g = torch.Generator().manual_seed(29)
    numel = n * h * h
    x = torch.randn(n, 1, h, h, generator=g)
    mask = known = None
    if mk is not None:
        mask = (torch.rand(1 if mk == "bcast" else n, 1, h, h, generator=g) < 0.5).float()
        mask[:, :, h // 2 - 2: h // 2 + 2] = 0.25
        known = torch.randn(n, 1, h, h, generator=g)
        known[(mask == 0).expand_as(known)] = float("nan")
    xi = torch.randn(Pn if fresh else 1, numel, generator=g)
    zeta = torch.randn(Pn - 1, numel, generator=g)
    xi_d, zeta_d = xi.cuda(), zeta.cuda()
    xi_nan, zeta_nan = torch.full_like(xi_d, float("nan")), torch.full_like(zeta_d, float("nan"))
    slots = torch.full((Pn + 1,), -1, dtype=torch.int32)
    slots[[11, 9, 6, 2, 1]] = torch.tensor([0, 3, 1, 4, 2], dtype=torch.int32)          # 9 and 6 jump, 11, 2, 1 do not
    nslots = 5
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    land_d, fa_d, fb_d, slots_d = _i32(prog.land_t), fa.cuda(), fb.cuda(), slots.cuda()
    sab_d, somab_d = sab.cuda(), somab.cuda()
    known_d = None if mk is None else known.cuda()
    mask_d = None if mk is None else mask.cuda()

    def launch(pos, xbuf, snaps, xt, zt):
        cur_k.fill_(pos)
        lb.cdm_mask_blend_jump(_ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(known_d), _ptr(mask_d),
                               0 if mk is None else mask_d.numel(), _ptr(cur_k), _ptr(land_d), Pn, T,
                               _ptr(sab_d) if mk else None, _ptr(somab_d) if mk else None, _ptr(fa_d), _ptr(fb_d),
                               _ptr(xt), numel, 1 if fresh else 0, _ptr(zt), numel, 0, None, _ptr(slots_d), _ptr(snaps),
                               _stream())

    def fresh_bufs():
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        return xbuf, torch.full((nslots, numel), -5.0, device="cuda")

    jumped = 0
    for q, (i, j, u) in enumerate(tr):
        p = Pn - q
        assert (int(prog.from_t[p]), int(prog.land_t[p]), int(prog.up_t[p])) == (i, j, u)
        xbuf, snaps = fresh_bufs()
        launch(p, xbuf, snaps, xi_d if j >= 1 else xi_nan, zeta_d if u != j else zeta_nan)
        v = x
        if mk is not None:
            xi_ref = xi[Pn - p if fresh else 0].reshape(x.shape) if j >= 1 else None
            v = I.blend(x, known, mask, sab[j], somab[j], xi_ref, j)
        ref = v
        if u != j:
            jumped += 1
            assert float(fb[p]) != 0
            ref = RS.forward_jump(v, fa[p], fb[p], zeta[Pn - p].reshape(x.shape))
            assert not torch.equal(ref, v)
        else:
            assert float(fb[p]) == 0 and float(fa[p]) == 1
        assert torch.isfinite(ref).all()
        got = xbuf.cpu()
        assert torch.equal(got[:n], ref), p
        if cfg:
            assert torch.equal(got[n:], ref), p
        sn = snaps.cpu()
        for s in range(nslots):
            if s == int(slots[p]):
                assert torch.equal(sn[s], v.reshape(-1)), (p, s)
            else:
                assert (sn[s] == -5.0).all(), (p, s)
    assert jumped == 2 and tr[-1][1] == 0
    for pos in (0, Pn + 1, -3):
        xbuf, snaps = fresh_bufs()
        before = xbuf.clone()
        launch(pos, xbuf, snaps, xi_d, zeta_d)
        assert torch.equal(xbuf, before) and (snaps == -5.0).all(), pos


@pytest.mark.parametrize("cfg,shape", [(False, (2, 64)), (True, (2, 64)), (True, (3, 20)), (False, (3, 20))])
def test_ddim_step_pos_kernel_bit_exact(cfg, shape):
    """cdm_ddim_step_pos = tests/_ddim_ref.step on the tables of ddim_tables_from_pairs (eta = 1), bit for bit, at every
    position of the same 11-position program, the host z read from row P - p; the snapshot slot of the position holds the
    new x; a position outside 1..P writes nothing."""
    import cdm_amd
    lb = cdm_amd.lib()
    n, h = shape
    ab_t = R.make_schedule(T)[2]
    prog = cdm_amd.resample_program(ab_t, D.subsequence(T, 7), jump=2, resamples=2)
    Pn = prog.P
    cx, ce, sg = (torch.from_numpy(v) for v in cdm_amd.ddim_tables_from_pairs(ab_t, prog.from_t, prog.land_t, 1.0))
    g = torch.Generator().manual_seed(31)
    numel = n * h * h
    x = torch.randn(n, 1, h, h, generator=g)
    ec, eu = torch.randn(n, 1, h, h, generator=g), torch.randn(n, 1, h, h, generator=g)
    z = torch.randn(Pn - 1, numel, generator=g)
    w = torch.tensor(3.0)
    eps_d = torch.cat([ec, eu]).cuda() if cfg else ec.cuda()
    z_d, nan_d = z.cuda(), torch.full((Pn - 1, numel), float("nan"), device="cuda")
    slots = torch.full((Pn + 1,), -1, dtype=torch.int32)
    slots[[11, 5, 1]] = torch.tensor([1, 0, 2], dtype=torch.int32)
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    cx_d, ce_d, sg_d, slots_d = cx.cuda(), ce.cuda(), sg.cuda(), slots.cuda()

    def launch(pos, xbuf, snaps, zt):
        cur_k.fill_(pos)
        lb.cdm_ddim_step_pos(_ptr(xbuf), _ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(eps_d), 1 if cfg else 0,
                             3.0, _ptr(cur_k), _ptr(cx_d), _ptr(ce_d), _ptr(sg_d), Pn, _ptr(zt), numel, 0, None,
                             _ptr(slots_d), _ptr(snaps), _stream())

    def fresh_bufs():
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        return xbuf, torch.full((3, numel), -5.0, device="cuda")

    for p in range(Pn, 0, -1):
        xbuf, snaps = fresh_bufs()
        launch(p, xbuf, snaps, z_d if p > 1 else nan_d)
        assert (float(sg[p]) == 0) == (p == 1)
        ref = D.step(x, ec, eu if cfg else None, w, cx[p], ce[p], sg[p], z[Pn - p].reshape(x.shape) if p > 1 else None)
        got = xbuf.cpu()
        assert torch.isfinite(ref).all() and torch.equal(got[:n], ref), p
        if cfg:
            assert torch.equal(got[n:], ref), p
        sn = snaps.cpu()
        for s in range(3):
            assert torch.equal(sn[s], ref.reshape(-1)) if s == int(slots[p]) else (sn[s] == -5.0).all(), (p, s)
    for pos in (0, Pn + 1):
        xbuf, snaps = fresh_bufs()
        before = xbuf.clone()
        launch(pos, xbuf, snaps, z_d)
        assert torch.equal(xbuf, before) and (snaps == -5.0).all(), pos


def test_invalid_value():
    """Null required pointers and non-positive sizes return hipErrorInvalidValue with nothing launched (x keeps its
    bits); the binding raises on it."""
    import cdm_amd
    lb = cdm_amd.lib()
    numel = 3 * 20 * 20
    x = torch.randn(numel, generator=torch.Generator().manual_seed(1)).cuda()
    before = x.clone()
    known, mask = torch.zeros(numel, device="cuda"), torch.ones(400, device="cuda")
    tab = torch.tensor([1.0, 0.5], device="cuda")                # sab / somab for T = 1; fa for P = 1
    zero = torch.zeros(2, device="cuda")                         # fb: no jump
    land = torch.zeros(2, dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    good = dict(x=_ptr(x), x2=None, numel=numel, known=_ptr(known), mask=_ptr(mask), mask_numel=400, cur_k=_ptr(one),
                land_t=_ptr(land), npos=1, T=1, sab=_ptr(tab), somab=_ptr(tab), fa=_ptr(tab), fb=_ptr(zero), xi=None,
                xistride=0, fresh=0, zeta=None, zetastride=0, seed=0, seed_dev=None, slot=None, snaps=None,
                stream=_stream())
    raw = lb.raw("cdm_mask_blend_jump")
    bad = [dict(x=None), dict(numel=0), dict(numel=-4), dict(cur_k=None), dict(land_t=None), dict(fa=None),
           dict(fb=None), dict(npos=0), dict(T=0), dict(xistride=-1), dict(zetastride=-1), dict(slot=_ptr(land)),
           dict(known=None), dict(sab=None), dict(somab=None), dict(mask_numel=0), dict(mask_numel=500)]
    for b in bad:
        assert raw(*{**good, **b}.values()) == INVALID, b
    with pytest.raises(cdm_amd._lib.HipError):
        lb.cdm_mask_blend_jump(*{**good, "numel": 0}.values())
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    assert raw(*good.values()) == 0                              # the valid call: p = 1, j = 0, m = 1, no jump: x <- known
    assert torch.equal(x, known)
    # the position-keyed step
    eps = torch.zeros(numel, device="cuda")
    x.copy_(before)
    sgood = dict(xin=_ptr(x), x=_ptr(x), x2=None, numel=numel, eps=_ptr(eps), cfg=0, w=0.0, cur_k=_ptr(one), cx=_ptr(tab),
                 ce=_ptr(tab), sigma=_ptr(zero), npos=1, z=None, zstride=0, seed=0, seed_dev=None, slot=None, snaps=None,
                 stream=_stream())
    raw = lb.raw("cdm_ddim_step_pos")
    for b in (dict(xin=None), dict(x=None), dict(eps=None), dict(cur_k=None), dict(cx=None), dict(ce=None),
              dict(sigma=None), dict(npos=0), dict(numel=0), dict(numel=-1), dict(zstride=-1), dict(slot=_ptr(land))):
        assert raw(*{**sgood, **b}.values()) == INVALID, b
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    assert raw(*sgood.values()) == 0                             # cx[1] = 0.5, ce * 0, sigma = 0
    assert torch.equal(x, before * 0.5)


# ---------------------------------------------------------------------------------------------------------------
# 2. device noise
# ---------------------------------------------------------------------------------------------------------------
def test_device_noise_is_keyed_by_the_position():
    """uniform(100, 12), J = 3, R = 3 (P = 30): positions 30 and 27 both go 100 -> 92, positions 28 and 25 both go
    83 -> 75 and jump to 100.  Without host tables the kernels draw from Philox by position: the two visits of a pair get
    different z, different "fresh" xi and different zeta; the same position and key the same bits; another key other
    draws.

    zeta over M = n H W = 8192 elements of a constant state c (null mask): the kernel stores fa c + fb zeta, so
    |mean - fa c| <= 5 fb / sqrt(M) and |var / fb^2 - 1| <= 5 sqrt(2 / M): five standard errors of the mean and of the
    variance of M standard normals.  The sample correlation of two independent standard normal vectors is
    N(0, 1 / M): |corr| <= 5 / sqrt(M) for zeta at the two positions and for zeta against z of the same position (same
    stream number, another key domain).  The bounds are derived, not measured."""
    import cdm_amd
    lb = cdm_amd.lib()
    ab_t = R.make_schedule(T)[2]
    taus = D.subsequence(T, S)
    prog = cdm_amd.resample_program(ab_t, taus, jump=3, resamples=3)
    Pn = prog.P
    assert Pn == 30
    tri = lambda p: (int(prog.from_t[p]), int(prog.land_t[p]), int(prog.up_t[p]))      # noqa: E731
    assert tri(30) == tri(27) == (100, 92, 92) and tri(28) == tri(25) == (83, 75, 100)
    M = N * H * H
    assert M == 8192
    bar = 5 / np.sqrt(M)
    sab, somab = (torch.from_numpy(v).cuda() for v in cdm_amd.known_tables(ab_t))
    land_d, fa_d, fb_d = _i32(prog.land_t), torch.from_numpy(prog.fa).cuda(), torch.from_numpy(prog.fb).cuda()
    cx, ce, sg = (torch.from_numpy(v).cuda() for v in cdm_amd.ddim_tables_from_pairs(ab_t, prog.from_t, prog.land_t, 1.0))
    zero_d, ones_d = torch.zeros(M, device="cuda"), torch.ones(M, device="cuda")

    def cell(v, dt):
        return torch.full((1,), v, dtype=dt, device="cuda")

    def z_of(p, key):
        out = torch.full((M,), 3.0, device="cuda")
        cur_k, zseed = cell(p, torch.int32), cell(key, torch.int64)       # both alive until the kernel has run
        lb.cdm_ddim_step_pos(_ptr(zero_d), _ptr(out), None, M, _ptr(zero_d), 0, 0.0, _ptr(cur_k), _ptr(cx), _ptr(ce),
                             _ptr(sg), Pn, None, M, 1234, _ptr(zseed), None, None, _stream())
        return out.cpu().double() / float(sg[p])

    def blend_jump(p, key, c, masked, fresh=True):
        out = torch.full((M,), c, device="cuda")
        cur_k, zseed = cell(p, torch.int32), cell(key, torch.int64)       # both alive until the kernel has run
        lb.cdm_mask_blend_jump(_ptr(out), None, M, _ptr(zero_d) if masked else None, _ptr(ones_d) if masked else None,
                               M if masked else 0, _ptr(cur_k), _ptr(land_d), Pn, T, _ptr(sab) if masked else None,
                               _ptr(somab) if masked else None, _ptr(fa_d), _ptr(fb_d), None, M, 1 if fresh else 0, None,
                               M, 1234, _ptr(zseed), None, None, _stream())
        return out.cpu()

    # z
    z30, z27 = z_of(30, 99), z_of(27, 99)
    assert torch.equal(z30, z_of(30, 99)) and not torch.equal(z30, z_of(30, 100))
    assert abs(_corr(z30, z27)) <= bar and abs(z30.std().item() - 1) <= 5 / np.sqrt(2 * M)
    # "fresh" xi: known = 0, m = 1, no jump at 30 / 27 -> somab[92] xi
    xi30, xi27 = (blend_jump(p, 99, 3.0, True).double() / float(somab[92]) for p in (30, 27))
    assert torch.equal(xi30, blend_jump(30, 99, 3.0, True).double() / float(somab[92]))
    assert abs(_corr(xi30, xi27)) <= bar and abs(xi30.std().item() - 1) <= 5 / np.sqrt(2 * M)
    assert abs(_corr(xi30, z30)) <= bar
    fx30, fx27 = (blend_jump(p, 99, 3.0, True, fresh=False) for p in (30, 27))
    assert torch.equal(fx30, fx27)                                # "fixed": one xi for the run
    # zeta
    c = 0.75
    outs = {}
    for p in (28, 25):
        fa, fb = float(prog.fa[p]), float(prog.fb[p])
        o = blend_jump(p, 99, c, False).double()
        mean, var = o.mean().item(), o.var().item()
        print(f"zeta p={p}: fa={fa:.6f} fb={fb:.6f} mean-fa*c={mean - fa * c:+.3e} (bar {5 * fb / np.sqrt(M):.3e}) "
              f"var/fb^2-1={var / fb ** 2 - 1:+.3e} (bar {5 * np.sqrt(2 / M):.3e})")
        assert abs(mean - fa * c) <= 5 * fb / np.sqrt(M)
        assert abs(var / fb ** 2 - 1) <= 5 * np.sqrt(2 / M)
        outs[p] = (o - fa * c) / fb
    assert torch.equal(blend_jump(28, 99, c, False), blend_jump(28, 99, c, False))
    assert not torch.equal(blend_jump(28, 99, c, False), blend_jump(28, 100, c, False))
    r1, r2 = _corr(outs[28], outs[25]), _corr(outs[28], z_of(28, 99))
    print(f"corr zeta28/zeta25 {r1:+.3e}, zeta28/z28 {r2:+.3e} (bar {bar:.3e})")
    assert abs(r1) <= bar and abs(r2) <= bar
    # a position that does not jump leaves a null-mask state alone
    assert torch.equal(blend_jump(30, 99, c, False), torch.full((M,), c))


# ---------------------------------------------------------------------------------------------------------------
# 3. exact properties of a run
# ---------------------------------------------------------------------------------------------------------------
def _call(d, kind, *a, **kw):
    if kind == "ddim":
        return d.sample_ddim(*a, steps=S, **kw)
    return d.sample_dpm(*a, steps=S, **kw)


@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_exact_properties_of_a_run(model, kind):
    """(a) An all-one mask with R = 2, J = 3 returns ``known`` bit for bit (the jumps re-noise it, the last blend lands on
    j = 0).  (b) resample=1, jump=1, t_start=None given explicitly: the same cache entry as the call without them and
    bit-equal output and snapshots.  (c) refine(t_start = T, noise=) equals sample_*_from_noise on
    sab[T] init + somab[T] noise, bit for bit (host z, DDIM at eta = 1: the RNG walks agree)."""
    import cdm_amd
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    params, known, w = _params(), _known(), 3.0
    opt = dict(eta=1.0) if kind == "ddim" else dict(order=2)
    torch.manual_seed(5)
    x1, i1 = _call(d, kind, N, H, None, params, w, known=known, mask=torch.ones(N, 1, H, H), known_noise="fresh",
                   resample=2, jump=3, **opt)
    assert torch.equal(x1.cpu(), known) and i1.shape[0] == cdm_amd.diffusion.snapshot_slots(21, 20)[1]
    # (b)
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    mask = _half_plane()
    torch.manual_seed(6)
    xa, ia = _call(d, kind, N, H, None, params, w, known=known, mask=mask, **opt)
    smp = next(iter(d._samplers.values()))
    torch.manual_seed(6)
    xb, ib = _call(d, kind, N, H, None, params, w, known=known, mask=mask, resample=1, jump=1, t_start=None, **opt)
    assert len(d._samplers) == 1 and next(iter(d._samplers.values())) is smp and smp.program is None
    assert torch.equal(xa, xb) and np.array_equal(ia, ib)
    # (c)
    g = torch.Generator().manual_seed(9)
    init, noise = torch.rand(N, 1, H, H, generator=g), torch.randn(N, 1, H, H, generator=g)
    sab, somab = (torch.from_numpy(v).cuda() for v in cdm_amd.known_tables(d.sched.ab_t))
    x_T = sab[T] * init.cuda() + somab[T] * noise.cuda()
    from_noise = d.sample_ddim_from_noise if kind == "ddim" else d.sample_dpm_from_noise
    torch.manual_seed(7)
    xr, ir = d.refine(init, T, params, w, sampler=kind, noise=noise, steps=S, **opt)
    torch.manual_seed(7)
    xn, inn = from_noise(x_T, params, steps=S, guide_w=w, **opt)
    assert len(d._samplers) == 3                                  # (b)'s, the late-start program's, the plain one
    assert torch.isfinite(xr).all() and torch.equal(xr, xn) and np.array_equal(ir, inn)


# ---------------------------------------------------------------------------------------------------------------
# 4. trajectory parity
# ---------------------------------------------------------------------------------------------------------------
def _rms(a, b, sel):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[sel]
    return float(np.sqrt(np.mean(d * d)))


TRAJ = [
    # kind, eta / order, w, known noise (None: unmasked), J, R, t_start
    ("ddim", 0.0, 0.0, "fixed", 3, 2, None),
    ("ddim", 1.0, 3.0, "fresh", 2, 3, None),
    ("dpmpp", 2, 0.0, "fixed", 3, 2, None),
    ("ddim", 0.0, 0.0, None, 1, 1, 60),
    ("dpmpp", 2, 0.0, "fixed", 3, 2, 60),
]


@pytest.mark.parametrize("kind,opt,w,mode,J,R_,t_start", TRAJ,
                         ids=["ddim-eta0-J3R2", "ddim-eta1-w3-fresh-J2R3", "dpmpp2-J3R2", "ddim-late60", "dpmpp2-late60-J3R2"])
def test_trajectory_matches_restatement(model, kind, opt, w, mode, J, R_, t_start):
    """CPU-RNG replay (z_source="host") of a program run, T = 100, S = 12 uniform, half-plane hard mask broadcast over the
    batch: the HIP sampler against the loops of tests/_resample_ref.py over the CPU oracle's forward, run in fp32 and, on
    the identical draws, in fp64 (the method and bar of test_gpu_inpaint.test_trajectory_matches_restatement).  At the
    final x and at every snapshot, HIP's RMS deviation from the fp64 run <= 3x the fp32 restatement's, the RMS taken over
    the generated region (m = 0), over all pixels in the unmasked late start.  Every ratio is recorded."""
    import cdm_amd
    seed = 7400
    sd = _sd()
    sched = R.make_schedule(T)
    ab_t = sched[2]
    taus = D.subsequence(T, S)
    prog = RS.program(taus, J, R_, t_start)
    params = _params()
    known = _known(43) if mode else None
    mask = _half_plane() if mode else None
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    fn32 = R.make_model_fn(sd, n_feat=NF, n_cfeat=NCF, height=H)

    def fn64(xx, t, cc):
        wgt, bias = R.draw_shortcut(1, NF)
        with torch.no_grad():
            return R.unet_forward(sd64, xx, t.double(), cc, n_feat=NF, n_cfeat=NCF, height=H, train=False,
                                  shortcut=(wgt.double(), bias.double()))

    def restate(fn, dt):
        torch.manual_seed(seed)
        x_T = torch.randn(N, 1, H, H).to(dt)
        loop = RS.ddim_loop if kind == "ddim" else RS.dpmpp_loop
        return loop(fn, x_T, params.to(dt), w, T, ab_t, prog, opt, known, mask, mode or "fixed")
    x32, inter32 = restate(fn32, torch.float32)
    x64, inter64 = restate(fn64, torch.float64)
    assert x32.dtype == torch.float32 and x64.dtype == torch.float64
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host", sched_tensors=sched)
    kw = dict(eta=opt) if kind == "ddim" else dict(order=opt)
    if mode:
        kw.update(known=known, mask=mask, known_noise=mode)
    torch.manual_seed(seed)
    x, inter = _call(d, kind, N, H, None, params, w, resample=R_, jump=J, t_start=t_start, **kw)
    assert x.shape == (N, 1, H, H) and inter.shape == tuple(inter32.shape)
    assert inter.shape[0] == cdm_amd.diffusion.snapshot_slots(len(prog), 20)[1]
    sel = np.ones((N, 1, H, H), dtype=bool)
    if mode:
        keep = (mask == 1).expand(N, 1, H, H)
        assert torch.equal(x.cpu()[keep], known[keep]) and torch.equal(x32[keep], known[keep])
        sel = (~keep).numpy()
    rows = [("final", _rms(x.cpu().numpy(), x64.numpy(), sel), _rms(x32.numpy(), x64.numpy(), sel))]
    for q in range(inter.shape[0]):
        rows.append((q, _rms(inter[q], inter64[q].numpy(), sel), _rms(inter32[q].numpy(), inter64[q].numpy(), sel)))
    worst = max(h / r for _, h, r in rows)
    name = f"{kind} opt={opt} w={w:g} {mode} J={J} R={R_} t_start={t_start}"
    print(f"resample trajectory {name}: rms deviation from fp64, HIP / fp32 restatement: "
          + " ".join(f"{a}:{h:.3e}/{r:.3e}" for a, h, r in rows) + f"; worst ratio {worst:.3f}")
    _parity.record("resample_trajectory", sampler=kind, T=T, S=S, P=len(prog), w=w, known_noise=mode, jump=J,
                   resample=R_, t_start=t_start, worst_ratio=worst, rms_x=float(x64.double().pow(2).mean().sqrt()),
                   points=[{"at": a, "hip": h, "ref32": r, "ratio": h / r} for a, h, r in rows], **kw_plain(kind, opt))
    for a, h, r in rows:
        assert h <= 3 * r, f"{name} at {a}: HIP {h:.3e} vs fp32 restatement {r:.3e}"


def kw_plain(kind, opt):
    return dict(eta=opt) if kind == "ddim" else dict(order=opt)


# ---------------------------------------------------------------------------------------------------------------
# 5. graph replay == eager
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog_kw,P_,replays", [(dict(resample=2, jump=3), 21, 2), (dict(t_start=60), 7, 0)])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_graph_replay_equals_eager(model, kind, prog_kw, P_, replays):
    """steps_per_graph = 10: P = 21 is two replays and one eager step, the late start's P = 7 is all eager; both equal
    use_graph=False bit for bit (final x and snapshots) with inpainting ("fresh", device noise, a soft-edged mask), CFG,
    DDIM at eta = 0.5 and DPM-Solver++ at order 2.  The per-run Philox key is pinned with torch.cuda.manual_seed."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = _params(1)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2))
    known, mask = _known(), _half_plane(N)
    mask[..., H // 2 - 2: H // 2] = 0.5
    outs = []
    for use_graph in (True, False):
        kw = dict(z_source="device", seed=11, use_graph=use_graph, steps_per_graph=10, inpaint="fresh", mask_n=N, **prog_kw)
        if kind == "ddim":
            smp = cdm_amd.DDIMSampler(model, sched, N, 3.0, params, steps=S, eta=0.5, **kw)
        else:
            smp = cdm_amd.DPMSolverSampler(model, sched, N, 3.0, params, steps=S, order=2, **kw)
        assert smp.npos == P_ and smp.program.P == P_ and smp.sc_table.shape[0] == P_
        torch.manual_seed(4)
        smp.prepare_rng(host_z=False)
        torch.cuda.manual_seed(8)
        x, inter = smp.run(xT, known=known, mask=mask)
        assert (smp.graph is not None) == (use_graph and replays > 0)
        assert smp.ctr.item() == 0
        outs.append((x.cpu(), inter))
    keep = mask == 1
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][0][keep], known[keep])
    assert torch.equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][1].shape[0] == cdm_amd.diffusion.snapshot_slots(P_, 20)[1]


# ---------------------------------------------------------------------------------------------------------------
# 6. reuse and determinism
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("ddim", "fresh"), ("dpmpp", "fixed")])
def test_second_call_reuses_sampler_and_graph(model, kind, mode):
    """Two resampled calls (R = 2, J = 3) with different known / mask contents of one shape: one cached sampler, one
    captured graph object, and the second result equals a fresh DDPM's for those inputs bit for bit (nothing stale in xi,
    zeta, known, mask or dprev).  z_source="host".  Another program is another sampler."""
    import cdm_amd
    params = _params()
    kA, kB = _known(51), _known(52)
    mA = _half_plane(N)
    mB = (torch.rand(N, 1, H, H, generator=torch.Generator().manual_seed(53)) < 0.3).float()
    mB[:, :, :4] = 0.5
    opt = dict(eta=1.0) if kind == "ddim" else {}
    opt.update(known_noise=mode, resample=2, jump=3)
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    torch.manual_seed(61)
    xa, _ = _call(d, kind, N, H, None, params, 3.0, known=kA, mask=mA, **opt)
    assert len(d._samplers) == 1
    smp = next(iter(d._samplers.values()))
    graph = smp.graph
    assert graph is not None and smp.npos == 21 and smp.zeta_table is not None
    torch.manual_seed(62)
    xb, ib = _call(d, kind, N, H, None, params, 3.0, known=kB, mask=mB, **opt)
    assert len(d._samplers) == 1 and next(iter(d._samplers.values())) is smp and smp.graph is graph
    fresh = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    torch.manual_seed(62)
    xf, i_f = _call(fresh, kind, N, H, None, params, 3.0, known=kB, mask=mB, **opt)
    assert not torch.equal(xa, xb)
    assert torch.equal(xb, xf) and np.array_equal(ib, i_f)
    _call(d, kind, N, H, None, params, 3.0, known=kB, mask=mB, **{**opt, "jump": 2})
    assert len(d._samplers) == 2
    _call(d, kind, N, H, None, params, 3.0, known=kB, mask=mB, **{**opt, "t_start": 60})
    assert len(d._samplers) == 3


def test_device_noise_determinism(model):
    """z_source="device", DDIM at eta = 1, "fresh", R = 2, J = 3, the shortcut table held fixed: two runs under the same
    torch.cuda.manual_seed agree bit for bit; under another seed z, xi and zeta change, so the generated region differs
    while the known pixels at the end are ``known``."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = _params(3)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(4))
    known, mask = _known(), _half_plane()
    smp = cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=S, eta=1.0, z_source="device", inpaint="fresh",
                              mask_n=1, resample=2, jump=3)
    assert smp.xi_table is None and smp.z_table is None and smp.zeta_table is None
    torch.manual_seed(6)
    smp.prepare_rng(host_z=False)
    outs = []
    for cs in (1, 1, 2):
        torch.cuda.manual_seed(cs)
        x, inter = smp.run(xT, known=known, mask=mask)
        outs.append((x.cpu(), inter))
    keep = (mask == 1).expand(N, 1, H, H)
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])
    for x, _ in outs:
        assert torch.equal(x[keep], known[keep])
    assert (outs[0][0][~keep] != outs[2][0][~keep]).any()


# ---------------------------------------------------------------------------------------------------------------
# 7. public interface
# ---------------------------------------------------------------------------------------------------------------
def test_api_shapes_and_snapshot_count(model):
    import cdm_amd
    for name in ("resample_program", "ddim_tables_from_pairs", "dpmpp_tables_from_pairs", "Program"):
        assert getattr(cdm_amd, name) is getattr(cdm_amd.diffusion, name)
    d = cdm_amd.DDPM(model, T, "cuda")
    params, known, mask = _params(8), _known(), _half_plane()
    keep = (mask == 1).expand(N, 1, H, H)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2)).cuda()
    slots = lambda P_, rate=20: cdm_amd.diffusion.snapshot_slots(P_, rate)[1]           # noqa: E731

    def ok(x, inter, nsnap, masked=True):
        assert x.shape == (N, 1, H, H) and x.is_cuda and torch.isfinite(x).all()
        assert inter.shape == (nsnap, N, 1, H, H) and np.isfinite(inter).all()
        assert np.array_equal(inter[-1], x.cpu().numpy())
        if masked:
            assert torch.equal(x.cpu()[keep], known[keep])
    ipk = dict(known=known, mask=mask)
    torch.manual_seed(1)
    ok(*d.sample_ddim(N, H, None, params, 0.0, steps=12, resample=2, jump=3, **ipk), slots(21))
    ok(*d.sample_ddim_from_noise(xT, params, steps=12, eta=0.5, guide_w=3.0, known_noise="fresh", resample=3, jump=2,
                                 save_rate=5, **ipk), slots(32, 5))
    ok(*d.sample_dpm(N, H, None, None, 3.0, steps=12, order=2, resample=2, jump=1, **ipk), slots(12 + 11))
    ok(*d.sample_dpm_from_noise(xT, None, steps=12, t_start=60, resample=2, jump=3, **ipk), slots(10))
    ok(*d.sample_ddim_from_noise(xT, params, steps=12, t_start=60), slots(7), masked=False)
    ok(*d.inpaint(known, mask, params, 3.0, sampler="ddim", steps=12, eta=1.0, resample=2, jump=3), slots(21))
    ok(*d.inpaint(known, mask, params, sampler="dpmpp", steps=12, resample=2, jump=3, t_start=70), slots(8 + 3))
    ok(*d.refine(known, 60, params, steps=12), slots(7), masked=False)
    ok(*d.refine(known, 60, params, 3.0, sampler="dpmpp", steps=12, **ipk), slots(7))
    ok(*d.refine(known.cuda(), 99, None, sampler="ddim", noise=torch.zeros(N, 1, H, H), steps=12, eta=1.0, resample=2,
                 jump=3, **ipk), slots(11 + 6))
    # errors, raised before anything is drawn or built
    nsmp = len(d._samplers)
    torch.manual_seed(77)
    state = torch.get_rng_state()
    for call in (lambda: d.inpaint(known, mask, params, sampler="ddpm", resample=2, jump=3),
                 lambda: d.inpaint(known, mask, params, sampler="ddpm", t_start=60),
                 lambda: d.refine(known, 60, params, sampler="ddpm")):
        with pytest.raises(ValueError, match='sampler="ddim", eta=1.0'):
            call()
    for call in (lambda: d.sample_ddim(N, H, None, params, 0.0, steps=12, resample=2, jump=3),       # no known / mask
                 lambda: d.sample_dpm_from_noise(xT, params, steps=12, resample=2, jump=3),
                 lambda: d.sample_ddim(N, H, None, params, 0.0, steps=12, resample=2, jump=7, **ipk),  # no jump point
                 lambda: d.sample_ddim(N, H, None, params, 0.0, steps=12, t_start=0),
                 lambda: d.sample_ddim(N, H, None, params, 0.0, steps=12, t_start=T + 1),
                 lambda: d.sample_dpm(N, H, None, params, 0.0, steps=12, t_start=5),                  # below tau_1 = 8
                 lambda: d.sample_dpm(N, H, None, params, 0.0, steps=12, jump=0, **ipk),
                 lambda: d.refine(known, 0, params, steps=12),
                 lambda: d.refine(known[:, 0], 60, params, steps=12),
                 lambda: d.refine(known, 60, params, steps=12, noise=torch.zeros(1, 1, H, H)),
                 lambda: d.refine(known, 60, params, sampler="euler"),
                 lambda: d.refine(known, 60, params, steps=12, known=known)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(torch.get_rng_state(), state) and len(d._samplers) == nsmp
    sched = cdm_amd.Schedule(T, "cuda")
    with pytest.raises(ValueError):
        cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=12, resample=2, jump=3)              # no mask
    with pytest.raises(ValueError):
        cdm_amd.DPMSolverSampler(model, sched, N, 0.0, params, steps=100, inpaint="fixed", resample=2)   # P > T


def test_in_channels_raise():
    import cdm_amd
    m = cdm_amd.ContextUnet(3, NF, NCF, H).cuda()
    d = cdm_amd.DDPM(m, 10, "cuda")
    known, mask = _known(), _half_plane()
    with pytest.raises(ValueError, match="in_channels"):
        d.sample_ddim(N, H, "cuda", torch.zeros(N, NCF).cuda(), 0.0, steps=5, known=known, mask=mask, resample=2)
    with pytest.raises(ValueError, match="in_channels"):
        d.sample_dpm_from_noise(torch.zeros(N, 3, H, H).cuda(), None, steps=5, t_start=6)
    with pytest.raises(ValueError, match="in_channels"):
        d.refine(known, 6, None, steps=5)
    with pytest.raises(ValueError, match="in_channels"):
        cdm_amd.DDIMSampler(m, d.sched, N, 0.0, None, steps=5, t_start=6)


def test_cli_resample_and_refine(tmp_path):
    """One run with --synthetic 8, one epoch, T = 100, --sample-steps 12: --inpaint-resample 2 --inpaint-jump 3 writes
    inpainted_samples.npy (known pixels kept) and names the 21 positions in its log line; --refine-init /
    --refine-t-start 60 writes refined_samples.npy and one Refinement line."""
    g = np.random.default_rng(5)
    known = g.random((2, 64, 64), dtype=np.float32)
    mask = np.zeros((64, 64), dtype=np.float32)
    mask[:, :24] = 1
    np.save(tmp_path / "known.npy", known); np.save(tmp_path / "mask.npy", mask)
    np.save(tmp_path / "init.npy", g.random((2, 1, 64, 64), dtype=np.float32))
    out_root = tmp_path / "out"
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "100", "6", "--synthetic", "8", "--n-feat", "16",
                        "--batch-size", "8", "--n-samples", "2", "--out-root", str(out_root), "--sample-steps", "12",
                        "--inpaint-known", str(tmp_path / "known.npy"), "--inpaint-mask", str(tmp_path / "mask.npy"),
                        "--inpaint-resample", "2", "--inpaint-jump", "3",
                        "--refine-init", str(tmp_path / "init.npy"), "--refine-t-start", "60"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = out_root / os.listdir(out_root)[0]
    filled = np.load(out / "inpainted_samples.npy")
    assert filled.shape == (2, 1, 64, 64) and np.isfinite(filled).all()
    assert np.array_equal(filled[:, 0, :, :24], known[:, :, :24])
    assert not np.array_equal(filled[:, 0, :, 24:], known[:, :, 24:])
    refined = np.load(out / "refined_samples.npy")
    assert refined.shape == (2, 1, 64, 64) and np.isfinite(refined).all()
    log = open(out / "timing_and_performance.log").read()
    inp = [ln for ln in log.splitlines() if ln.startswith("Inpainting")]
    ref = [ln for ln in log.splitlines() if ln.startswith("Refinement of")]
    assert len(inp) == 1 and "resample=2, jump=3, 21 positions" in inp[0] and "T=100, steps=12, eta=0:" in inp[0], log
    assert len(ref) == 1 and "t_start=60" in ref[0] and "T=100, steps=12, eta=0:" in ref[0], log
