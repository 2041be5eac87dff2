"""Strided DDIM sampling (eta, CFG) on the graph-captured sampler: kernels, trajectory parity, determinism, graph
replay, public interface and CLI.  The definition is tests/_ddim_ref.py (the reference has no DDIM).

Shapes: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64), n = 2, T = 100 unless a test says otherwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
import _parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
NF, NCF, H, N, T = 8, 6, 64, 2, 100


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


# ---------------------------------------------------------------------------------------------------------------
# 1. the fused update kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, 3.0])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_step_kernel_bit_exact(eta, w):
    """cdm_ddim_step = separate fp32 torch-CPU ops on the same fp32 tables, bit for bit: the new x, the second half of
    the model-input buffer (CFG), the snapshot slot written (and no other), z row S - k of the table; at every position of
    a uniform(100, 7) table, the last included (sigma = 0: z is not read, a NaN row there must not matter)."""
    import cdm_amd
    lb = cdm_amd.lib()
    S = 7
    taus = cdm_amd.timestep_subsequence(T, S, "uniform")
    assert taus == D.subsequence(T, S)
    _, _, ab_t = R.make_schedule(T)
    cx, ce, sg = (torch.from_numpy(v) for v in cdm_amd.ddim_tables(ab_t, taus, eta))
    for mine, ref in zip((cx, ce, sg), D.coefficients(ab_t, taus, eta)):
        assert torch.equal(mine, ref)
    cfg = w > 0
    g = torch.Generator().manual_seed(17)
    numel = N * H * H
    x, ec, eu = (torch.randn(N, 1, H, H, generator=g) for _ in range(3))
    ztab = torch.randn(S - 1, numel, generator=g)
    ztab_d = torch.cat([ztab, torch.full((1, numel), float("nan"))]).cuda()    # row S - 1 belongs to k = 1: never read
    slots = torch.tensor([-1, 3, -1, 0, -1, 2, -1, 1], dtype=torch.int32)      # by position k
    nslots = 4
    eps_d = (torch.cat([ec, eu]) if cfg else ec).cuda().contiguous()
    cur_i = torch.zeros(1, dtype=torch.int32, device="cuda")
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    cxd, ced, sgd, slots_d = cx.cuda(), ce.cuda(), sg.cuda(), slots.cuda()
    for k in range(S, 0, -1):
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        snaps = torch.full((nslots, numel), -5.0, device="cuda")
        cur_i.fill_(taus[k - 1]); cur_k.fill_(k)
        lb.cdm_ddim_step(_ptr(xbuf), _ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(eps_d), 1 if cfg else 0,
                         float(w), _ptr(cur_i), _ptr(cur_k), _ptr(cxd), _ptr(ced), _ptr(sgd), S, _ptr(ztab_d), numel,
                         0, None, _ptr(slots_d), _ptr(snaps), _stream())
        z = ztab[S - k].reshape(x.shape) if k > 1 else None
        if eta == 0 or k == 1:
            assert float(sg[k]) == 0.0
        else:
            assert float(sg[k]) > 0.0
        ref = D.step(x, ec, eu if cfg else None, torch.tensor(w), cx[k], ce[k], sg[k], z)
        got = xbuf.cpu()
        assert torch.equal(got[:N], ref), (k, eta, w)
        if cfg:
            assert torch.equal(got[N:], ref), (k, eta, w)
        sn = snaps.cpu()
        for s in range(nslots):
            if s == int(slots[k]):
                assert torch.equal(sn[s], ref.reshape(-1)), (k, s)
            else:
                assert (sn[s] == -5.0).all(), (k, s)


def test_ddim_step_kernel_device_z():
    """Without a z table the kernel draws z from Philox, keyed by the per-run key and the timestep: (v - mean) / sigma is
    standard normal (mean / std of 8192 draws within 6 standard errors), the same for the same key and timestep, different
    for another timestep or key; sigma = 0 draws nothing."""
    import cdm_amd
    lb = cdm_amd.lib()
    S = 7
    taus = cdm_amd.timestep_subsequence(T, S)
    _, _, ab_t = R.make_schedule(T)
    cx, ce, sg = (torch.from_numpy(v) for v in cdm_amd.ddim_tables(ab_t, taus, 1.0))
    g = torch.Generator().manual_seed(18)
    numel = N * H * H
    x, ec = torch.randn(N, 1, H, H, generator=g), torch.randn(N, 1, H, H, generator=g)
    xd, ed = x.cuda(), ec.cuda()
    cxd, ced, sgd = cx.cuda(), ce.cuda(), sg.cuda()
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(k, i, key):
        out = torch.empty_like(xd)
        cur_i = torch.full((1,), i, dtype=torch.int32, device="cuda")
        cur_k.fill_(k)
        zseed = torch.full((1,), key, dtype=torch.int64, device="cuda")
        lb.cdm_ddim_step(_ptr(xd), _ptr(out), None, numel, _ptr(ed), 0, 0.0, _ptr(cur_i), _ptr(cur_k), _ptr(cxd),
                         _ptr(ced), _ptr(sgd), S, None, numel, 1234, _ptr(zseed), None, None, _stream())
        return out.cpu()
    k = 4
    mean = cx[k] * x + ce[k] * ec
    a = run(k, taus[k - 1], 99)
    z = ((a - mean) / sg[k]).double().reshape(-1)
    assert abs(z.mean().item()) < 6 / np.sqrt(numel) and abs(z.std().item() - 1) < 6 / np.sqrt(2 * numel)
    assert torch.equal(a, run(k, taus[k - 1], 99))
    assert not torch.equal(a, run(k, taus[k - 1] + 1, 99))
    assert not torch.equal(a, run(k, taus[k - 1], 100))
    assert torch.equal(run(1, taus[0], 99), cx[1] * x + ce[1] * ec)


# ---------------------------------------------------------------------------------------------------------------
# 2. the strided prologue
# ---------------------------------------------------------------------------------------------------------------
def test_prologue_sub_kernel():
    """Five launches over a 5-position table: cur_i = steps[k], cur_k = k, t_cur = fp32(i / T), shortcut row S - k, the
    counter counts down to 0; a launch past the last position writes nothing."""
    import cdm_amd
    lb = cdm_amd.lib()
    S, T_, row = 5, 20, 2 * 2 * NF
    steps = [0, 3, 7, 12, 16, 20]
    steps_d = torch.tensor(steps, dtype=torch.int32).cuda()
    table = torch.randn(S, row, generator=torch.Generator().manual_seed(5))
    table_d = table.cuda()
    ctr = torch.full((1,), S, dtype=torch.int32, device="cuda")
    cur_i = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    cur_k = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    t_cur = torch.zeros(1, device="cuda")
    sc_cur = torch.zeros(row, device="cuda")

    def launch():
        lb.cdm_sample_prologue_sub(_ptr(ctr), S, T_, _ptr(steps_d), _ptr(cur_i), _ptr(cur_k), _ptr(t_cur),
                                   _ptr(table_d), row, _ptr(sc_cur), _stream())
    for k in range(S, 0, -1):
        launch()
        assert cur_i.item() == steps[k] and cur_k.item() == k
        assert ctr.item() == k - 1
        assert torch.equal(t_cur.cpu(), torch.tensor([steps[k] / T_]))
        assert torch.equal(sc_cur.cpu(), table[S - k])
    assert ctr.item() == 0
    launch()
    assert ctr.item() == 0 and cur_i.item() == steps[1] and cur_k.item() == 1
    assert torch.equal(sc_cur.cpu(), table[S - 1])


# ---------------------------------------------------------------------------------------------------------------
# 3. trajectory parity
# ---------------------------------------------------------------------------------------------------------------
def _rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("eta,w", [(0.0, 0.0), (1.0, 0.0), (0.0, 3.0)])
def test_trajectory_matches_restatement(model, eta, w):
    """S = 12 uniform over T = 100, CPU-RNG replay (z_source="host"): DDIMSampler against tests/_ddim_ref.sample_loop over
    the CPU oracle's forward, run in fp32 and — on the identical draws — in fp64 (state dict, inputs and schedule cast to
    double as tests/golden/make_golden_r5.py does).  Bar: at the final x and at each of the 8 snapshots, HIP's RMS
    deviation from the fp64 run <= 3x the fp32 restatement's own (a 12-step run is forward-error dominated; 1.5x is kept
    for the 400-1500-step trajectories where per-step errors average out).  The golden weights are an init, not a
    trained model: a ReLU / MaxPool branch flip in one fp32 run can dominate its deviation.  Every ratio is recorded."""
    import cdm_amd
    S, seed = 12, 7100
    sd = _sd()
    b_t, a_t, ab_t = R.make_schedule(T)
    taus = D.subsequence(T, S)
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(31))
    # fp32 restatement
    torch.manual_seed(seed)
    x_T = torch.randn(N, 1, H, H)
    fn32 = R.make_model_fn(sd, n_feat=NF, n_cfeat=NCF, height=H)
    x32, inter32 = D.sample_loop(fn32, x_T, params, w, T, ab_t, taus, eta)
    # fp64 on the same draws
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}

    def fn64(xx, t, cc):
        wgt, bias = R.draw_shortcut(1, NF)
        with torch.no_grad():
            return R.unet_forward(sd64, xx, t.double(), cc, n_feat=NF, n_cfeat=NCF, height=H, train=False,
                                  shortcut=(wgt.double(), bias.double()))
    torch.manual_seed(seed)
    x_T64 = torch.randn(N, 1, H, H)
    assert torch.equal(x_T64, x_T)
    x64, inter64 = D.sample_loop(fn64, x_T64.double(), params.double(), w, T, ab_t, taus, eta)
    # HIP
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host", sched_tensors=(b_t, a_t, ab_t))
    torch.manual_seed(seed)
    x, inter = d.sample_ddim(N, H, None, params, w, steps=S, eta=eta, spacing="uniform")
    assert x.shape == (N, 1, H, H) and inter.shape == (8, N, 1, H, H) == tuple(inter32.shape)
    rows = [("final", _rms(x.cpu().numpy(), x64.numpy()), _rms(x32.numpy(), x64.numpy()))]
    for j in range(inter.shape[0]):
        rows.append((j, _rms(inter[j], inter64[j].numpy()), _rms(inter32[j].numpy(), inter64[j].numpy())))
    worst = max(h / r for _, h, r in rows)
    print(f"ddim trajectory eta={eta:g} w={w:g}: rms deviation from fp64, HIP / fp32 restatement: "
          + " ".join(f"{a}:{h:.3e}/{r:.3e}" for a, h, r in rows) + f"; worst ratio {worst:.3f}")
    _parity.record("ddim_trajectory_S12_T100", eta=eta, w=w, worst_ratio=worst, rms_x=float(x64.double().pow(2).mean().sqrt()),
                   points=[{"at": a, "hip": h, "ref32": r, "ratio": h / r} for a, h, r in rows])
    for a, h, r in rows:
        assert h <= 3 * r, f"eta={eta:g} w={w:g} at {a}: HIP {h:.3e} vs fp32 restatement {r:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# 4. determinism at eta = 0
# ---------------------------------------------------------------------------------------------------------------
def test_eta0_is_deterministic_eta1_is_not(model):
    """z_source="device", the shortcut table held fixed, the same x_T, different torch.cuda.manual_seed: eta = 0 gives
    the same bits (no z is drawn), eta = 1 does not."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(3))
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(4))
    for eta, same in ((0.0, True), (1.0, False)):
        smp = cdm_amd.DDIMSampler(model, sched, N, 0.0, params, steps=12, eta=eta, z_source="device")
        torch.manual_seed(6)
        smp.prepare_rng(host_z=False)
        outs = []
        for cs in (1, 2):
            torch.cuda.manual_seed(cs)
            x, inter = smp.run(xT)
            outs.append((x.cpu(), inter))
        assert torch.isfinite(outs[0][0]).all()
        assert torch.equal(outs[0][0], outs[1][0]) == same, eta
        assert np.array_equal(outs[0][1], outs[1][1]) == same, eta


# ---------------------------------------------------------------------------------------------------------------
# 5. graph replay == eager
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,replays", [(13, 2), (3, 0)])
def test_graph_replay_equals_eager(model, S, replays):
    """steps_per_graph = 5: S = 13 is two replays and three eager steps, S = 3 is all eager; both equal use_graph=False
    bit for bit (final x and snapshots), with CFG and eta = 0.5 (device z)."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(1))
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2))
    outs = []
    for use_graph in (True, False):
        smp = cdm_amd.DDIMSampler(model, sched, N, 3.0, params, steps=S, eta=0.5, z_source="device", seed=11,
                                  use_graph=use_graph, steps_per_graph=5)
        torch.manual_seed(4)
        smp.prepare_rng(host_z=False)
        x, inter = smp.run(xT)
        assert (smp.graph is not None) == (use_graph and replays > 0)
        assert smp.ctr.item() == 0
        outs.append((x.cpu(), inter))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][1].shape[0] == cdm_amd.diffusion.snapshot_slots(S, 20)[1]


# ---------------------------------------------------------------------------------------------------------------
# 6. public interface
# ---------------------------------------------------------------------------------------------------------------
def test_api_shapes_and_snapshot_count(model):
    import cdm_amd
    d = cdm_amd.DDPM(model, T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(1)
    x, inter = d.sample_ddim(N, H, None, params, 0.0, steps=12)
    assert x.shape == (N, 1, H, H) and x.is_cuda and torch.isfinite(x).all()
    assert inter.shape == (8, N, 1, H, H)                       # positions 12 and 7..1
    assert np.array_equal(inter[-1], x.cpu().numpy())
    x, inter = d.sample_ddim(N, H, None, None, 3.0, steps=25, eta=1.0, spacing="quadratic", save_rate=5)
    assert x.shape == (N, 1, H, H) and inter.shape == (11, N, 1, H, H)      # 25, 20, 15, 10 and 7..1
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2)).cuda()
    x, inter = d.sample_ddim_from_noise(xT, params, steps=6, eta=0.5, guide_w=3.0)
    assert x.shape == (N, 1, H, H) and inter.shape == (6, N, 1, H, H) and np.isfinite(inter).all()
    x, inter = d.sample_ddim_from_noise(xT, None, steps=None, spacing=[2, 50, 100])
    assert x.shape == (N, 1, H, H) and inter.shape == (3, N, 1, H, H)
    assert len(d._samplers) == 4
    d.sample_ddim_from_noise(xT, params, steps=6, eta=0.5, guide_w=3.0)
    assert len(d._samplers) == 4                                 # cached by (steps, eta, spacing)
    d.sample_ddim_from_noise(xT, params, steps=6, eta=0.25, guide_w=3.0)
    assert len(d._samplers) == 5
    with pytest.raises(ValueError):
        d.sample_ddim(N, H, None, params, 0.0, steps=T + 1)


def test_functional_sampler_steps(model):
    """sample_ddpm(..., steps=12) is DDPM.sample_ddim under the same seed; steps=None is the ancestral path, bit for bit."""
    import cdm_amd
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(8))
    for p in (params, None):
        torch.manual_seed(9)
        a = cdm_amd.sample_ddpm(model, N, H, "cuda", p, 0.0, T, steps=12, eta=0.5, spacing="quadratic")
        torch.manual_seed(9)
        b, _ = cdm_amd.DDPM(model, T, "cuda").sample_ddim(N, H, None, p, 0.0, steps=12, eta=0.5, spacing="quadratic")
        assert a.shape == (N, 1, H, H) and torch.equal(a, b)
    T_ = 12
    torch.manual_seed(10)
    a = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T_, steps=None)
    torch.manual_seed(10)
    b = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T_)
    torch.manual_seed(10)
    c, _ = cdm_amd.DDPM(model, T_, "cuda").sample_ddpm(N, H, None, params, 0.0)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_in_channels_raise():
    import cdm_amd
    m = cdm_amd.ContextUnet(3, NF, NCF, H).cuda()
    d = cdm_amd.DDPM(m, 10, "cuda")
    with pytest.raises(NotImplementedError):
        d.sample_ddim(2, H, "cuda", torch.zeros(2, NCF).cuda(), 0.0, steps=5)
    with pytest.raises(NotImplementedError):
        d.sample_ddim_from_noise(torch.zeros(2, 3, H, H).cuda(), None, steps=5)


# ---------------------------------------------------------------------------------------------------------------
# 7. CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_sample_steps(tmp_path):
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "20", "6", "--synthetic", "150", "--n-feat", "16",
                        "--batch-size", "16", "--n-samples", "3", "--out-root", str(tmp_path), "--sample-steps", "5",
                        "--eta", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / os.listdir(tmp_path)[0]
    rec = np.load(out / "reconstructed_images.npy")
    assert rec.shape == (3, 1, 64, 64) and np.isfinite(rec).all()
    inter = np.load(out / "intermediate.npy")
    assert inter.shape == (5, 3, 1, 64, 64) and np.isfinite(inter).all()
    gen = np.load(out / "generated_samples.npy")
    assert gen.shape == (3, 1, 64, 64) and np.isfinite(gen).all()
    log = open(out / "timing_and_performance.log").read()
    lines = [ln for ln in log.splitlines() if ln.startswith(("Reconstruction", "Sampling"))]
    assert len(lines) == 2 and all("T=20, steps=5, eta=0:" in ln for ln in lines), log
