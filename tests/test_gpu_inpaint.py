"""Masked (inpainting) sampling on the graph-captured samplers: the blend kernel, its device noise, exact properties of a
run, trajectory parity, graph replay, determinism, buffer reuse, public interface and CLI.  The definition is
tests/_inpaint_ref.py (the reference has no inpainting).

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
import _dpmpp_ref as P
import _inpaint_ref as I
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
    """Hard mask: the left half of every map is known."""
    m = torch.zeros(n, 1, H, H)
    m[..., : H // 2] = 1
    return m


def _known(seed=41, n=N):
    return torch.rand(n, 1, H, H, generator=torch.Generator().manual_seed(seed))


def _params(seed=31):
    return torch.rand(N, NCF, generator=torch.Generator().manual_seed(seed))


def _sample(d, kind, params, w, **kw):
    """One call of the DDPM method of a sampler kind, S positions for the strided ones."""
    if kind == "ddpm":
        return d.sample_ddpm(N, H, None, params, w, **kw)
    if kind == "ddim":
        return d.sample_ddim(N, H, None, params, w, steps=S, **kw)
    return d.sample_dpm(N, H, None, params, w, steps=S, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. the blend kernel
# ---------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    # form, cfg, broadcast mask, fresh, (n, h)
    ("ancestral", False, False, True, (2, 64)),
    ("ancestral", True, True, False, (2, 64)),
    ("ancestral", True, False, True, (2, 64)),
    ("ancestral", False, True, False, (2, 64)),
    ("strided", False, False, False, (2, 64)),
    ("strided", True, True, True, (2, 64)),
    ("strided", True, False, False, (2, 64)),
    ("strided", False, True, True, (2, 64)),
    ("strided", True, False, True, (3, 20)),       # 1200 elements: the grid-stride tail (a last block partly filled)
    ("ancestral", False, True, False, (3, 20)),
]


@pytest.mark.parametrize("form,cfg,bcast,fresh,shape", KERNEL_CASES)
def test_mask_blend_kernel_bit_exact(form, cfg, bcast, fresh, shape):
    """cdm_mask_blend = tests/_inpaint_ref.blend (separate fp32 torch-CPU ops on the same fp32 tables), bit for bit, at
    every position of a 7-position run, the last (j = 0) included: the new x, the second half of the model-input buffer
    (CFG), the snapshot slot named for the position (and no other), xi row rows - position ("fresh") or 0 ("fixed").
    The mask is hard (0 / 1 at random) with a soft 0.25 band, per sample or broadcast; ``known`` is NaN wherever its
    mask is 0 (never read there); at j = 0 the whole xi table is NaN (never read).  Strided form: uniform(100, 7);
    ancestral form: T = 7.  A position outside 1..7, or i outside 1..T, writes nothing."""
    import cdm_amd
    lb = cdm_amd.lib()
    n, h = shape
    S_ = 7
    strided = form == "strided"
    T_ = T if strided else S_
    ab_t = R.make_schedule(T_)[2]
    taus = D.subsequence(T_, S_) if strided else list(range(1, S_ + 1))
    steps = [0] + taus
    sab, somab = (torch.from_numpy(v) for v in cdm_amd.known_tables(ab_t))
    for mine, ref in zip((sab, somab), I.tables(ab_t)):
        assert torch.equal(mine, ref)
    g = torch.Generator().manual_seed(23)
    numel = n * h * h
    x = torch.randn(n, 1, h, h, generator=g)
    mn = 1 if bcast else n
    mask = (torch.rand(mn, 1, h, h, generator=g) < 0.5).float()
    mask[:, :, h // 2 - 2: h // 2 + 2] = 0.25
    assert set(mask.unique().tolist()) == {0.0, 0.25, 1.0}
    known = torch.randn(n, 1, h, h, generator=g)
    known[(mask == 0).expand_as(known)] = float("nan")
    rows = S_ if fresh else 1
    xi = torch.randn(rows, numel, generator=g)
    xi_d = xi.cuda()
    nan_d = torch.full((rows, numel), float("nan"), device="cuda")
    slots = torch.tensor([-1, 3, -1, 0, -1, 2, -1, 1], dtype=torch.int32)      # by position
    nslots = 4
    cur_i = torch.zeros(1, dtype=torch.int32, device="cuda")
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    steps_d = torch.tensor(steps, dtype=torch.int32).cuda()
    known_d, mask_d, sab_d, somab_d, slots_d = known.cuda(), mask.cuda(), sab.cuda(), somab.cuda(), slots.cuda()

    def launch(pos, i, xbuf, snaps, table):
        cur_i.fill_(i); cur_k.fill_(pos)
        lb.cdm_mask_blend(_ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(known_d), _ptr(mask_d), mask_d.numel(),
                          _ptr(cur_i), _ptr(cur_k) if strided else None, _ptr(steps_d) if strided else None, S_, T_,
                          _ptr(sab_d), _ptr(somab_d), _ptr(table), numel, 1 if fresh else 0, 0, None, _ptr(slots_d),
                          _ptr(snaps), _stream())

    def fresh_bufs():
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        return xbuf, torch.full((nslots, numel), -5.0, device="cuda")

    for pos in range(S_, 0, -1):
        i, j = steps[pos], steps[pos - 1]
        xbuf, snaps = fresh_bufs()
        launch(pos, i, xbuf, snaps, xi_d if j >= 1 else nan_d)
        xi_ref = xi[S_ - pos if fresh else 0].reshape(x.shape) if j >= 1 else None
        ref = I.blend(x, known, mask, sab[j], somab[j], xi_ref, j)
        assert torch.isfinite(ref).all()
        hard1, hard0 = (mask == 1).expand_as(x), (mask == 0).expand_as(x)
        kn = known if j == 0 else sab[j] * known + somab[j] * xi_ref
        assert torch.equal(ref[hard1], kn[hard1]) and torch.equal(ref[hard0], x[hard0])
        got = xbuf.cpu()
        assert torch.equal(got[:n], ref), (pos, form)
        if cfg:
            assert torch.equal(got[n:], ref), (pos, form)
        sn = snaps.cpu()
        for s in range(nslots):
            if s == int(slots[pos]):
                assert torch.equal(sn[s], ref.reshape(-1)), (pos, s)
            else:
                assert (sn[s] == -5.0).all(), (pos, s)
    outside = [(0, steps[1]), (S_ + 1, T_), (3, 0), (3, T_ + 1)] if strided else [(0, 0), (0, T_ + 1)]
    for pos, i in outside:
        xbuf, snaps = fresh_bufs()
        before = xbuf.clone()
        launch(pos, i, xbuf, snaps, xi_d)
        assert torch.equal(xbuf, before) and (snaps == -5.0).all(), (pos, i)


def test_mask_blend_invalid_value():
    """numel <= 0, mask_numel <= 0 and numel % mask_numel != 0 return hipErrorInvalidValue (nothing is launched: x
    keeps its bits); the binding raises on it."""
    import cdm_amd
    lb = cdm_amd.lib()
    numel = 3 * 20 * 20
    x = torch.randn(numel, generator=torch.Generator().manual_seed(1)).cuda()
    before = x.clone()
    known, mask = torch.zeros(numel, device="cuda"), torch.ones(numel, device="cuda")
    tab = torch.tensor([1.0, 0.5], device="cuda")
    cur_i = torch.ones(1, dtype=torch.int32, device="cuda")

    def args(ne, mne):
        return (_ptr(x), None, ne, _ptr(known), _ptr(mask), mne, _ptr(cur_i), None, None, 1, 1, _ptr(tab), _ptr(tab),
                None, 0, 0, 0, None, None, None, _stream())
    raw = lb.raw("cdm_mask_blend")
    for ne, mne in ((0, 400), (-4, 400), (numel, 0), (numel, -400), (numel, 500), (numel, numel + 1)):
        assert raw(*args(ne, mne)) == INVALID, (ne, mne)
    with pytest.raises(cdm_amd._lib.HipError):
        lb.cdm_mask_blend(*args(numel, 500))
    assert raw(*args(numel, 400)) == 0                      # the valid call: i = 1, j = 0, m = 1: x <- known
    assert torch.equal(x, known) and not torch.equal(before, known)


# ---------------------------------------------------------------------------------------------------------------
# 2. device noise
# ---------------------------------------------------------------------------------------------------------------
def test_mask_blend_device_noise():
    """Without an xi table the kernel draws xi from Philox.  On m = 1 pixels, (v - sab known) / somab: standard normal
    (mean / std of 8192 draws within 6 standard errors, the bar of test_ddim_step_kernel_device_z); the same bits for
    the same key and stream; "fixed" gives one xi at two different j, "fresh" two; another key another xi; and the draw
    is not the z cdm_ddim_step makes for the same key and stream number (the key domains differ).

    With known = 0 the kernel stores fl(somab xi), so v / somab evaluated in fp64 is xi (1 + d), |d| <= 2^-24: two
    recoveries of one xi differ by at most 2^-23 |xi|; independent standard normals have a sample correlation of
    N(0, 1 / 8192), bar 6 / sqrt(8192)."""
    import cdm_amd
    lb = cdm_amd.lib()
    S_ = 7
    taus = D.subsequence(T, S_)
    ab_t = R.make_schedule(T)[2]
    sab, somab = (torch.from_numpy(v) for v in cdm_amd.known_tables(ab_t))
    numel = N * H * H
    g = torch.Generator().manual_seed(19)
    known = torch.randn(numel, generator=g)
    zero_d, known_d, ones_d = torch.zeros(numel, device="cuda"), known.cuda(), torch.ones(numel, device="cuda")
    sab_d, somab_d = sab.cuda(), somab.cuda()
    steps_d = torch.tensor([0] + taus, dtype=torch.int32).cuda()

    def run(k, key, fresh, kn_d):
        out = torch.full((numel,), 3.0, device="cuda")
        cur_i = torch.full((1,), taus[k - 1], dtype=torch.int32, device="cuda")
        cur_k = torch.full((1,), k, dtype=torch.int32, device="cuda")
        zseed = torch.full((1,), key, dtype=torch.int64, device="cuda")
        lb.cdm_mask_blend(_ptr(out), None, numel, _ptr(kn_d), _ptr(ones_d), numel, _ptr(cur_i), _ptr(cur_k),
                          _ptr(steps_d), S_, T, _ptr(sab_d), _ptr(somab_d), None, numel, 1 if fresh else 0, 1234,
                          _ptr(zseed), None, None, _stream())
        return out.cpu()

    def xi_of(v, k):
        return v.double() / somab[taus[k - 2]].double()

    k = 5
    j = taus[k - 2]
    a = run(k, 99, True, known_d)
    xi = ((a.double() - sab[j].double() * known.double()) / somab[j].double())
    assert abs(xi.mean().item()) < 6 / np.sqrt(numel) and abs(xi.std().item() - 1) < 6 / np.sqrt(2 * numel)
    assert torch.equal(a, run(k, 99, True, known_d))
    assert not torch.equal(a, run(k, 100, True, known_d))
    f5, f3 = xi_of(run(5, 99, False, zero_d), 5), xi_of(run(3, 99, False, zero_d), 3)
    assert (f5 - f3).abs().le(2.0 ** -23 * f5.abs()).all()             # "fixed": one xi at two different j
    r5, r3 = xi_of(run(5, 99, True, zero_d), 5), xi_of(run(3, 99, True, zero_d), 3)
    corr = lambda u, v: float(((u - u.mean()) * (v - v.mean())).mean() / (u.std() * v.std()))    # noqa: E731
    bar = 6 / np.sqrt(numel)
    assert abs(corr(r5, r3)) < bar and abs(corr(r5, f5)) < bar          # "fresh": another stream per j, none of them 0
    assert abs(corr(r5, xi_of(run(5, 100, True, zero_d), 5))) < bar
    assert abs(r5.std().item() - 1) < 6 / np.sqrt(2 * numel) and abs(f5.std().item() - 1) < 6 / np.sqrt(2 * numel)
    # z of cdm_ddim_step at the timestep i = j of the blend above (stream j on both sides), same seed and per-run key
    cx, ce, sg = (torch.from_numpy(v).cuda() for v in cdm_amd.ddim_tables(ab_t, taus, 1.0))
    kz = k - 1
    assert taus[kz - 1] == j and float(sg[kz]) > 0
    out = torch.empty(numel, device="cuda")
    cur_i = torch.full((1,), j, dtype=torch.int32, device="cuda")
    cur_k = torch.full((1,), kz, dtype=torch.int32, device="cuda")
    zseed = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    lb.cdm_ddim_step(_ptr(zero_d), _ptr(out), None, numel, _ptr(zero_d), 0, 0.0, _ptr(cur_i), _ptr(cur_k), _ptr(cx),
                     _ptr(ce), _ptr(sg), S_, None, numel, 1234, _ptr(zseed), None, None, _stream())
    z = out.cpu().double() / float(sg[kz])
    assert abs(z.std().item() - 1) < 6 / np.sqrt(2 * numel)
    assert abs(corr(r5, z)) < bar and abs(corr(f5, z)) < bar
    # j = 0 draws nothing: x <- known exactly
    assert torch.equal(run(1, 99, True, known_d), known)


# ---------------------------------------------------------------------------------------------------------------
# 3. exact properties of a run
# ---------------------------------------------------------------------------------------------------------------
def _build(cdm_amd, kind, model, sched, params, w, **kw):
    if kind == "ddpm":
        return cdm_amd.GraphSampler(model, sched, N, w, params, z_source="host", **kw)
    if kind == "ddim":
        return cdm_amd.DDIMSampler(model, sched, N, w, params, steps=S, eta=1.0, z_source="host", **kw)
    return cdm_amd.DPMSolverSampler(model, sched, N, w, params, steps=S, order=2, z_source="host", **kw)


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmpp"])
def test_exact_properties_of_a_run(model, kind):
    """(a) Hard half-plane mask: the final x equals ``known`` bit for bit wherever m = 1, and differs from it elsewhere.
    (b) All-one mask: the run returns ``known`` exactly.  (c) All-zero mask: final x and snapshots bit-identical to the
    same sampler built without inpainting, on the same host z and shortcut draws (the plain sampler's tables, drawn
    under one CPU seed, copied into the masked one: its own prepare_rng draws xi first, which shifts every later draw
    of the stream).  In (c) DDIM runs at eta = 1 so z is in play; CFG on throughout."""
    import cdm_amd
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    params, known, w = _params(), _known(), 3.0
    mask = _half_plane()
    torch.manual_seed(5)
    x, inter = _sample(d, kind, params, w, known=known, mask=mask)
    x = x.cpu()
    keep = (mask == 1).expand_as(x)
    assert torch.isfinite(x).all() and torch.equal(x[keep], known[keep])
    assert (x[~keep] != known[~keep]).float().mean() > 0.99
    assert np.array_equal(inter[-1], x.numpy())
    torch.manual_seed(5)
    x1, _ = _sample(d, kind, params, w, known=known, mask=torch.ones(N, 1, H, H), known_noise="fresh")
    assert torch.equal(x1.cpu(), known)
    # (c) on the samplers themselves
    sched = cdm_amd.Schedule(T, "cuda")
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2))
    plain = _build(cdm_amd, kind, model, sched, params, w)
    torch.manual_seed(6)
    plain.prepare_rng(host_z=True)
    xp, ip = plain.run(xT)
    for mode, mn in (("fixed", 1), ("fresh", N)):
        masked = _build(cdm_amd, kind, model, sched, params, w, inpaint=mode, mask_n=mn)
        torch.manual_seed(6)
        masked.prepare_rng(host_z=True)
        masked.sc_table.copy_(plain.sc_table)
        if plain.z_table is not None:
            masked.z_table.copy_(plain.z_table)
        xm, im = masked.run(xT, known=known, mask=torch.zeros(mn, 1, H, H))
        assert torch.equal(xm, xp) and np.array_equal(im, ip), (kind, mode)


# ---------------------------------------------------------------------------------------------------------------
# 4. trajectory parity
# ---------------------------------------------------------------------------------------------------------------
def _rms(a, b, sel):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[sel]
    return float(np.sqrt(np.mean(d * d)))


TRAJ = [("ddpm", dict(), 0.0, "fixed"), ("ddim", dict(eta=0.0), 0.0, "fixed"), ("ddim", dict(eta=1.0), 3.0, "fresh"),
        ("dpmpp", dict(order=2), 0.0, "fixed")]


@pytest.mark.parametrize("kind,opt,w,mode", TRAJ, ids=["ddpm", "ddim-eta0", "ddim-eta1-w3-fresh", "dpmpp2"])
def test_trajectory_matches_restatement(model, kind, opt, w, mode):
    """CPU-RNG replay (z_source="host") of a masked run, T = 100 (ancestral: all 100 steps; strided: S = 12 uniform),
    half-plane hard mask broadcast over the batch, ``known`` drawn once from a seeded generator: the HIP sampler against
    the loops of tests/_inpaint_ref.py over the CPU oracle's forward, run in fp32 and, on the identical draws, in fp64
    (the method of test_gpu_ddim.test_trajectory_matches_restatement).  Bar, that test's own: at the final x and at
    every snapshot, HIP's RMS deviation from the fp64 run <= 3x the fp32 restatement's, the RMS taken over the generated
    region (m = 0) only: the known region is exact at the end and would dilute the ratio.  Every ratio is recorded."""
    import cdm_amd
    seed = 7300
    sd = _sd()
    sched = R.make_schedule(T)
    b_t, a_t, ab_t = sched
    taus = D.subsequence(T, S)
    params = _params()
    known = _known(43)
    mask = _half_plane()
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
        p = params.to(dt)
        if kind == "ddpm":
            return I.ancestral_loop(fn, x_T, p, w, T, tuple(v.to(dt) for v in sched), known, mask, mode)
        if kind == "ddim":
            return I.ddim_loop(fn, x_T, p, w, T, ab_t, taus, opt["eta"], known, mask, mode)
        tabs = cdm_amd.dpmpp_tables(ab_t, taus, opt["order"])
        return I.dpmpp_loop(fn, x_T, p, w, T, ab_t, taus, tabs, known, mask, mode)
    x32, inter32 = restate(fn32, torch.float32)
    x64, inter64 = restate(fn64, torch.float64)
    assert x32.dtype == torch.float32 and x64.dtype == torch.float64
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host", sched_tensors=sched)
    torch.manual_seed(seed)
    x, inter = _sample(d, kind, params, w, known=known, mask=mask, known_noise=mode, **opt)
    assert x.shape == (N, 1, H, H) and inter.shape == tuple(inter32.shape)
    keep = (mask == 1).expand(N, 1, H, H)
    assert torch.equal(x.cpu()[keep], known[keep]) and torch.equal(x32[keep], known[keep])
    gen = (~keep).numpy()
    rows = [("final", _rms(x.cpu().numpy(), x64.numpy(), gen), _rms(x32.numpy(), x64.numpy(), gen))]
    for q in range(inter.shape[0]):
        rows.append((q, _rms(inter[q], inter64[q].numpy(), gen), _rms(inter32[q].numpy(), inter64[q].numpy(), gen)))
    worst = max(h / r for _, h, r in rows)
    print(f"inpaint trajectory {kind} {opt} w={w:g} {mode}: rms deviation from fp64 on m = 0, HIP / fp32 restatement: "
          + " ".join(f"{a}:{h:.3e}/{r:.3e}" for a, h, r in rows) + f"; worst ratio {worst:.3f}")
    _parity.record("inpaint_trajectory", sampler=kind, T=T, S=(T if kind == "ddpm" else S), w=w, known_noise=mode,
                   worst_ratio=worst, rms_x=float(x64.double().pow(2).mean().sqrt()),
                   points=[{"at": a, "hip": h, "ref32": r, "ratio": h / r} for a, h, r in rows], **opt)
    for a, h, r in rows:
        assert h <= 3 * r, f"{kind} {opt} w={w:g} {mode} at {a}: HIP {h:.3e} vs fp32 restatement {r:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# 5. graph replay == eager
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_,replays", [(13, 2), (3, 0)])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_graph_replay_equals_eager(model, kind, S_, replays):
    """steps_per_graph = 5: S = 13 is two replays and three eager steps, S = 3 is all eager; both equal use_graph=False
    bit for bit (final x and snapshots) with inpainting on ("fresh", device noise, a soft-edged mask), CFG, DDIM at
    eta = 0.5 and DPM-Solver++ at order 2.  The per-run Philox key is pinned with torch.cuda.manual_seed."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = _params(1)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2))
    known, mask = _known(), _half_plane(N)
    mask[..., H // 2 - 2: H // 2] = 0.5
    outs = []
    for use_graph in (True, False):
        kw = dict(z_source="device", seed=11, use_graph=use_graph, steps_per_graph=5, inpaint="fresh", mask_n=N)
        if kind == "ddim":
            smp = cdm_amd.DDIMSampler(model, sched, N, 3.0, params, steps=S_, eta=0.5, **kw)
        else:
            smp = cdm_amd.DPMSolverSampler(model, sched, N, 3.0, params, steps=S_, order=2, **kw)
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
    assert outs[0][1].shape[0] == cdm_amd.diffusion.snapshot_slots(S_, 20)[1]


# ---------------------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------------------
def test_device_noise_determinism(model):
    """z_source="device", DDIM at eta = 0 (no z), "fixed", the shortcut table held fixed: two runs under the same
    torch.cuda.manual_seed agree bit for bit; under another seed only xi changes, so the runs differ (in the generated
    region, and in the snapshots) while the known pixels at the end are the same: ``known``."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = _params(3)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(4))
    known, mask = _known(), _half_plane()
    smp = cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=S, eta=0.0, z_source="device", inpaint="fixed",
                              mask_n=1)
    assert smp.xi_table is None and smp.z_table is None
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
    assert not torch.equal(outs[0][0], outs[2][0]) and not np.array_equal(outs[0][1][0], outs[2][1][0])
    for x, _ in outs:
        assert torch.equal(x[keep], known[keep])
    assert (outs[0][0][~keep] != outs[2][0][~keep]).any()


# ---------------------------------------------------------------------------------------------------------------
# 7. buffer reuse
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("ddim", "fresh"), ("dpmpp", "fixed"), ("ddpm", "fixed")])
def test_second_call_reuses_sampler_and_graph(model, kind, mode):
    """Two calls with different known / mask contents of one shape: one cached sampler, one captured graph object, and
    the second result equals a fresh DDPM's result for those inputs bit for bit (nothing stale in xi, known, mask or
    dprev).  z_source="host", the same CPU seed for the second call and the fresh one."""
    import cdm_amd
    params = _params()
    kA, kB = _known(51), _known(52)
    mA = _half_plane(N)
    mB = (torch.rand(N, 1, H, H, generator=torch.Generator().manual_seed(53)) < 0.3).float()
    mB[:, :, :4] = 0.5
    opt = dict(eta=1.0) if kind == "ddim" else {}
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    torch.manual_seed(61)
    xa, _ = _sample(d, kind, params, 3.0, known=kA, mask=mA, known_noise=mode, **opt)
    assert len(d._samplers) == 1
    smp = next(iter(d._samplers.values()))
    graph = smp.graph
    assert graph is not None and smp.inpaint == mode and smp.mask_n == N
    torch.manual_seed(62)
    xb, ib = _sample(d, kind, params, 3.0, known=kB, mask=mB, known_noise=mode, **opt)
    assert len(d._samplers) == 1 and next(iter(d._samplers.values())) is smp and smp.graph is graph
    fresh = cdm_amd.DDPM(model, T, "cuda", z_source="host")
    torch.manual_seed(62)
    xf, i_f = _sample(fresh, kind, params, 3.0, known=kB, mask=mB, known_noise=mode, **opt)
    assert not torch.equal(xa, xb)
    assert torch.equal(xb, xf) and np.array_equal(ib, i_f)
    # another noise mode or mask extent is another sampler
    _sample(d, kind, params, 3.0, known=kB, mask=mB[:1], known_noise=mode, **opt)
    assert len(d._samplers) == 2
    _sample(d, kind, params, 3.0, known=kB, mask=mB, known_noise="fresh" if mode == "fixed" else "fixed", **opt)
    assert len(d._samplers) == 3
    _sample(d, kind, params, 3.0, **opt)
    assert len(d._samplers) == 4 and sum(s.inpaint is None for s in d._samplers.values()) == 1


# ---------------------------------------------------------------------------------------------------------------
# 8. public interface
# ---------------------------------------------------------------------------------------------------------------
def test_api_shapes_and_snapshot_count(model):
    import cdm_amd
    assert cdm_amd.known_tables is cdm_amd.diffusion.known_tables
    assert cdm_amd.check_inpaint is cdm_amd.diffusion.check_inpaint
    d = cdm_amd.DDPM(model, T, "cuda")
    params, known, mask = _params(8), _known(), _half_plane()
    keep = (mask == 1).expand(N, 1, H, H)
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2)).cuda()

    def ok(x, inter, nsnap):
        assert x.shape == (N, 1, H, H) and x.is_cuda and torch.isfinite(x).all()
        assert inter.shape == (nsnap, N, 1, H, H) and np.isfinite(inter).all()
        assert np.array_equal(inter[-1], x.cpu().numpy())
        assert torch.equal(x.cpu()[keep], known[keep])
    torch.manual_seed(1)
    ok(*d.sample_ddim(N, H, None, params, 0.0, steps=12, known=known, mask=mask), 8)
    ok(*d.sample_ddim_from_noise(xT, params, steps=6, eta=0.5, guide_w=3.0, known=known.cuda(), mask=mask.cuda(),
                                 known_noise="fresh"), 6)
    ok(*d.sample_dpm(N, H, None, None, 3.0, steps=25, order=2, spacing="quadratic", save_rate=5, known=known,
                     mask=mask.expand(N, 1, H, H)), 11)
    ok(*d.sample_dpm_from_noise(xT, None, steps=None, spacing=[2, 50, 100], known=known, mask=mask), 3)
    ok(*d.sample_ddpm(N, H, None, params, 0.0, known=known, mask=mask), 12)             # 100, 80, 60, 40, 20 and 7..1
    ok(*d.sample_ddpm_from_noise(xT, params, guide_w=3.0, known=known.double(), mask=mask.numpy()), 12)
    assert len(d._samplers) == 6 and all(s.inpaint is not None for s in d._samplers.values())
    ok(*d.inpaint(known, mask), 12)
    ok(*d.inpaint(known, mask, params, 3.0, sampler="ddim", steps=12, eta=1.0, known_noise="fresh"), 8)
    ok(*d.inpaint(known, mask, params, sampler="dpmpp", steps=6, order=1), 6)
    # DDPM.inpaint draws x_T as the matching sample_* method does (the CUDA seed pins the device xi)
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    a, _ = d.inpaint(known, mask, params, 0.0, sampler="dpmpp", steps=12)
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    b, _ = d.sample_dpm(N, H, None, params, 0.0, steps=12, known=known, mask=mask)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="sampler"):
        d.inpaint(known, mask, sampler="euler")


def test_functional_sampler_known_mask(model):
    """sample_ddpm(..., known=, mask=) is the DDPM method of the selected sampler under the same seeds (device noise:
    the CPU and the CUDA seed), bit for bit, on all four of its paths."""
    import cdm_amd
    params, known, mask = _params(8), _known(), _half_plane()
    keep = (mask == 1).expand(N, 1, H, H)
    T_ = 12

    def seeds():
        torch.manual_seed(9); torch.cuda.manual_seed(9)
    ipk = dict(known=known, mask=mask, known_noise="fresh")
    for extra, call in ((dict(steps=6, eta=0.5), lambda d, p: d.sample_ddim(N, H, None, p, 0.0, steps=6, eta=0.5, **ipk)),
                        (dict(steps=6, solver="dpmpp"), lambda d, p: d.sample_dpm(N, H, None, p, 0.0, steps=6, **ipk)),
                        (dict(), lambda d, p: d.sample_ddpm(N, H, None, p, 0.0, **ipk))):
        for p in (params, None):
            seeds()
            a = cdm_amd.sample_ddpm(model, N, H, "cuda", p, 0.0, T_, **extra, **ipk)
            seeds()
            b, _ = call(cdm_amd.DDPM(model, T_, "cuda"), p)
            assert a.shape == (N, 1, H, H) and torch.equal(a, b), (extra, p is None)
            assert torch.equal(a.cpu()[keep], known[keep])
    with pytest.raises(ValueError):
        cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T_, known=known)


def test_validation_errors(model):
    """Every ValueError of the keyword paths, raised before anything is drawn (the CPU RNG does not move) or built."""
    import cdm_amd
    d = cdm_amd.DDPM(model, T, "cuda")
    params, known, mask = _params(8), _known(), _half_plane()
    xT = torch.zeros(N, 1, H, H).cuda()
    bad_mask, nan_mask, nan_known = mask.clone(), mask.clone().cuda(), known.clone().cuda()
    bad_mask[0, 0, 0, 0] = 1.5
    nan_mask[0, 0, 3, 3] = float("nan")
    nan_known[1, 0, 0, 0] = float("inf")                    # column 0 is known
    torch.manual_seed(77)
    state = torch.get_rng_state()
    cases = [dict(known=known), dict(mask=mask), dict(known=known[:1], mask=mask), dict(known=known[:, 0], mask=mask),
             dict(known=known, mask=mask[..., :32]), dict(known=known, mask=torch.cat([mask] * 3)),
             dict(known=known, mask=bad_mask), dict(known=known.cuda(), mask=nan_mask),
             dict(known=nan_known, mask=mask.cuda()), dict(known=known, mask=mask, known_noise="repaint")]
    for kw in cases:
        for call in (lambda: d.sample_ddpm(N, H, None, params, 0.0, **kw),
                     lambda: d.sample_ddpm_from_noise(xT, params, **kw),
                     lambda: d.sample_ddim(N, H, None, params, 0.0, steps=5, **kw),
                     lambda: d.sample_ddim_from_noise(xT, params, steps=5, **kw),
                     lambda: d.sample_dpm(N, H, None, params, 0.0, steps=5, **kw),
                     lambda: d.sample_dpm_from_noise(xT, params, steps=5, **kw),
                     lambda: cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        d.inpaint(known, None)
    with pytest.raises(ValueError):
        d.inpaint(known[:, 0], mask)
    assert torch.equal(torch.get_rng_state(), state) and len(d._samplers) == 0
    # known may be anything where the mask is 0
    holes = known.clone()
    holes[..., H // 2:] = float("nan")
    x, _ = d.sample_ddim(N, H, None, params, 0.0, steps=5, known=holes, mask=mask)
    assert torch.isfinite(x).all()
    # the samplers refuse the keywords they were not built for
    sched = cdm_amd.Schedule(T, "cuda")
    plain = cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=5)
    masked = cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=5, inpaint="fixed", mask_n=1)
    with pytest.raises(ValueError):
        plain.run(xT, known=known, mask=mask)
    with pytest.raises(ValueError):
        masked.run(xT)
    with pytest.raises(ValueError):
        masked.run(xT, known=known)
    with pytest.raises(ValueError):
        cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=5, inpaint="repaint")
    with pytest.raises(ValueError):
        cdm_amd.GraphSampler(model, sched, N, 0.0, params, inpaint="fixed", mask_n=3)


def test_in_channels_raise():
    import cdm_amd
    m = cdm_amd.ContextUnet(3, NF, NCF, H).cuda()
    d = cdm_amd.DDPM(m, 10, "cuda")
    known, mask = _known(), _half_plane()
    with pytest.raises(ValueError, match="in_channels"):
        d.sample_ddim(N, H, "cuda", torch.zeros(N, NCF).cuda(), 0.0, steps=5, known=known, mask=mask)
    with pytest.raises(ValueError, match="in_channels"):
        d.sample_ddpm_from_noise(torch.zeros(N, 3, H, H).cuda(), None, known=known, mask=mask)
    with pytest.raises(ValueError, match="in_channels"):
        d.inpaint(known, mask, sampler="dpmpp", steps=5)
    with pytest.raises(ValueError, match="single-channel"):
        cdm_amd.GraphSampler(m, d.sched, N, 0.0, None, inpaint="fixed")


def test_cli_inpaint(tmp_path):
    """One run with --synthetic 8, one epoch, --sample-steps 5 and the two inpaint files: inpainted_samples.npy is
    written beside the usual outputs, its known pixels are the input file's, and the log names the run."""
    g = np.random.default_rng(5)
    known = g.random((2, 64, 64), dtype=np.float32)
    mask = np.zeros((64, 64), dtype=np.float32)
    mask[:, :24] = 1
    np.save(tmp_path / "known.npy", known); np.save(tmp_path / "mask.npy", mask)
    out_root = tmp_path / "out"
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "20", "6", "--synthetic", "8", "--n-feat", "16",
                        "--batch-size", "8", "--n-samples", "2", "--out-root", str(out_root), "--sample-steps", "5",
                        "--inpaint-known", str(tmp_path / "known.npy"), "--inpaint-mask", str(tmp_path / "mask.npy")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = out_root / os.listdir(out_root)[0]
    filled = np.load(out / "inpainted_samples.npy")
    assert filled.shape == (2, 1, 64, 64) and np.isfinite(filled).all()
    assert np.array_equal(filled[:, 0, :, :24], known[:, :, :24])
    assert not np.array_equal(filled[:, 0, :, 24:], known[:, :, 24:])
    assert np.load(out / "reconstructed_images.npy").shape == (2, 1, 64, 64)
    assert np.load(out / "generated_samples.npy").shape == (2, 1, 64, 64)
    log = open(out / "timing_and_performance.log").read()
    lines = [ln for ln in log.splitlines() if ln.startswith(("Reconstruction", "Sampling", "Inpainting"))]
    assert len(lines) == 3 and all("T=20, steps=5, eta=0:" in ln for ln in lines), log
    assert "fixed noise" in lines[2]
