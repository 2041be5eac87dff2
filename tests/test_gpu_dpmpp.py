"""Second-order multistep sampling (DPM-Solver++ 2M, CFG) on the graph-captured sampler: the update kernel, trajectory
parity, determinism and buffer reuse, graph replay, public interface and CLI.  The definition is tests/_dpmpp_ref.py
(the reference has no such sampler).

Shapes: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64), n = 2, T = 100 unless a test says otherwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
import _dpmpp_ref as P
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
@pytest.mark.parametrize("order", [1, 2])
def test_dpmpp_step_kernel_bit_exact(order, w):
    """cdm_dpmpp_step = separate fp32 torch-CPU ops on the same fp32 tables, bit for bit: the new x, the second half of
    the model-input buffer (CFG), dprev after the call, the snapshot slot written (and no other); at every position of a
    uniform(100, 7) table.  Where c1 = 0 (k = S, k = 1, every k at order 1) dprev holds NaN before the call: it must not
    be read.  A k of 0 or S + 1 leaves every buffer untouched."""
    import cdm_amd
    lb = cdm_amd.lib()
    S = 7
    taus = cdm_amd.timestep_subsequence(T, S, "uniform")
    assert taus == P.subsequence(T, S)
    _, _, ab_t = R.make_schedule(T)
    tabs = tuple(torch.from_numpy(v) for v in cdm_amd.dpmpp_tables(ab_t, taus, order))
    sq, ra, c0, c1, cx, cd = tabs
    for mine, ref in zip(tabs, P.coefficients(ab_t, taus, order)):
        assert torch.allclose(mine, ref, rtol=2.0 ** -22, atol=0)          # numpy's log vs libm's: the last fp32 bit at most
    cfg = w > 0
    g = torch.Generator().manual_seed(19)
    numel = N * H * H
    x, ec, eu, dp = (torch.randn(N, 1, H, H, generator=g) for _ in range(4))
    slots = torch.tensor([-1, 3, -1, 0, -1, 2, -1, 1], dtype=torch.int32)      # by position k
    nslots = 4
    eps_d = (torch.cat([ec, eu]) if cfg else ec).cuda().contiguous()
    cur_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    tabs_d = [t.cuda() for t in tabs]
    slots_d = slots.cuda()

    def launch(k, xbuf, dprev, snaps):
        cur_k.fill_(k)
        lb.cdm_dpmpp_step(_ptr(xbuf), _ptr(xbuf), _ptr(xbuf) if cfg else None, numel, _ptr(eps_d), 1 if cfg else 0,
                          float(w), _ptr(cur_k), *(_ptr(t) for t in tabs_d), S, _ptr(dprev), _ptr(slots_d), _ptr(snaps),
                          _stream())

    for k in range(S, 0, -1):
        first_order = order == 1 or k in (1, S)
        assert (float(c1[k]) == 0.0) == first_order and (float(c0[k]) == 1.0) == first_order
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        snaps = torch.full((nslots, numel), -5.0, device="cuda")
        dprev = torch.full((numel,), float("nan"), device="cuda") if first_order else dp.reshape(-1).clone().cuda()
        launch(k, xbuf, dprev, snaps)
        ref, d = P.step(x, ec, eu if cfg else None, torch.tensor(w), sq[k], ra[k], c0[k], c1[k], cx[k], cd[k], dp)
        got = xbuf.cpu()
        assert torch.isfinite(got[:N]).all(), (k, order, w)
        assert torch.equal(got[:N], ref), (k, order, w)
        if cfg:
            assert torch.equal(got[N:], ref), (k, order, w)
        assert torch.equal(dprev.cpu(), d.reshape(-1)), (k, order, w)
        sn = snaps.cpu()
        for s in range(nslots):
            if s == int(slots[k]):
                assert torch.equal(sn[s], ref.reshape(-1)), (k, s)
            else:
                assert (sn[s] == -5.0).all(), (k, s)
    for k in (0, S + 1):
        xbuf = torch.cat([x, torch.full_like(x, 7.0)]).cuda() if cfg else x.clone().cuda()
        before = xbuf.clone()
        snaps = torch.full((nslots, numel), -5.0, device="cuda")
        dprev = dp.reshape(-1).clone().cuda()
        launch(k, xbuf, dprev, snaps)
        assert torch.equal(xbuf, before) and torch.equal(dprev.cpu(), dp.reshape(-1)) and (snaps == -5.0).all(), k


# ---------------------------------------------------------------------------------------------------------------
# 2. trajectory parity
# ---------------------------------------------------------------------------------------------------------------
def _rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("order,w", [(2, 0.0), (2, 3.0), (1, 0.0)])
def test_trajectory_matches_restatement(model, order, w):
    """S = 12 uniform over T = 100, CPU-RNG replay (z_source="host"): DDPM.sample_dpm against
    tests/_dpmpp_ref.sample_loop over the CPU oracle's forward, run in fp32 and, on the identical draws and the same
    fp32 tables, in fp64 (state dict, inputs and tables cast to double, as test_gpu_ddim.py builds its fp64 run).
    Bar: at the final x and at each of the 8 snapshots, HIP's RMS deviation from the fp64 run <= 3x the fp32
    restatement's own: the bar of DDIM's 12-step test, for the reason its docstring gives (a 12-step run is
    forward-error dominated, and the golden weights are an init, so a ReLU / MaxPool branch flip in one fp32 run can
    dominate its deviation).  Every ratio is recorded."""
    import cdm_amd
    S, seed = 12, 7200
    sd = _sd()
    b_t, a_t, ab_t = R.make_schedule(T)
    taus = P.subsequence(T, S)
    tables = cdm_amd.dpmpp_tables(ab_t, taus, order)
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(31))
    # fp32 restatement
    torch.manual_seed(seed)
    x_T = torch.randn(N, 1, H, H)
    fn32 = R.make_model_fn(sd, n_feat=NF, n_cfeat=NCF, height=H)
    x32, inter32 = P.sample_loop(fn32, x_T, params, w, T, taus, tables)
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
    x64, inter64 = P.sample_loop(fn64, x_T64.double(), params.double(), w, T, taus, tables)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    # HIP
    d = cdm_amd.DDPM(model, T, "cuda", z_source="host", sched_tensors=(b_t, a_t, ab_t))
    torch.manual_seed(seed)
    x, inter = d.sample_dpm(N, H, None, params, w, steps=S, order=order, spacing="uniform")
    assert x.shape == (N, 1, H, H) and inter.shape == (8, N, 1, H, H) == tuple(inter32.shape)
    rows = [("final", _rms(x.cpu().numpy(), x64.numpy()), _rms(x32.numpy(), x64.numpy()))]
    for j in range(inter.shape[0]):
        rows.append((j, _rms(inter[j], inter64[j].numpy()), _rms(inter32[j].numpy(), inter64[j].numpy())))
    worst = max(h / r for _, h, r in rows)
    print(f"dpmpp trajectory order={order} w={w:g}: rms deviation from fp64, HIP / fp32 restatement: "
          + " ".join(f"{a}:{h:.3e}/{r:.3e}" for a, h, r in rows) + f"; worst ratio {worst:.3f}")
    _parity.record("dpmpp_trajectory_S12_T100", order=order, w=w, worst_ratio=worst,
                   rms_x=float(x64.double().pow(2).mean().sqrt()),
                   points=[{"at": a, "hip": h, "ref32": r, "ratio": h / r} for a, h, r in rows])
    for a, h, r in rows:
        assert h <= 3 * r, f"order={order} w={w:g} at {a}: HIP {h:.3e} vs fp32 restatement {r:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# 3. determinism and reuse of the sampler's buffers
# ---------------------------------------------------------------------------------------------------------------
def test_deterministic_and_no_stale_dprev(model):
    """The shortcut table held fixed: two run(x_T) calls on one sampler under different torch.cuda.manual_seed give the
    same bits (nothing is drawn on the device); and a run made right after a run from another x_T equals a fresh
    sampler's run of it (dprev left by the earlier run is not read at the first position)."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(3))
    xA = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(4))
    xB = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(5))

    def make():
        smp = cdm_amd.DPMSolverSampler(model, sched, N, 3.0, params, steps=12, order=2, z_source="device")
        torch.manual_seed(6)
        smp.prepare_rng(host_z=False)
        return smp
    smp = make()
    assert smp.z_table is None
    outs = []
    for cs in (1, 2):
        torch.cuda.manual_seed(cs)
        x, inter = smp.run(xA)
        outs.append((x.cpu(), inter))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    xb, ib = smp.run(xB)                                  # right after runs from xA
    fresh = make()
    xf, i_f = fresh.run(xB)
    assert not torch.equal(xb.cpu(), outs[0][0])
    assert torch.equal(xb, xf) and np.array_equal(ib, i_f)


# ---------------------------------------------------------------------------------------------------------------
# 4. graph replay == eager
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,replays", [(13, 2), (3, 0)])
def test_graph_replay_equals_eager(model, S, replays):
    """steps_per_graph = 5: S = 13 is two replays and three eager steps (a multistep boundary falls between two replays
    and between a replay and the tail), S = 3 is all eager; both equal use_graph=False bit for bit (final x and
    snapshots), with CFG and order 2."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(1))
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2))
    outs = []
    for use_graph in (True, False):
        smp = cdm_amd.DPMSolverSampler(model, sched, N, 3.0, params, steps=S, order=2, z_source="device", seed=11,
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
# 5. public interface
# ---------------------------------------------------------------------------------------------------------------
def test_api_shapes_and_snapshot_count(model):
    import cdm_amd
    assert cdm_amd.DPMSolverSampler is cdm_amd.diffusion.DPMSolverSampler
    assert cdm_amd.dpmpp_tables is cdm_amd.diffusion.dpmpp_tables
    d = cdm_amd.DDPM(model, T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(1)
    x, inter = d.sample_dpm(N, H, None, params, 0.0, steps=12)
    assert x.shape == (N, 1, H, H) and x.is_cuda and torch.isfinite(x).all()
    assert inter.shape == (8, N, 1, H, H)                       # positions 12 and 7..1
    assert np.array_equal(inter[-1], x.cpu().numpy())
    x, inter = d.sample_dpm(N, H, None, None, 3.0, steps=25, order=1, spacing="quadratic", save_rate=5)
    assert x.shape == (N, 1, H, H) and inter.shape == (11, N, 1, H, H)      # 25, 20, 15, 10 and 7..1
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2)).cuda()
    x, inter = d.sample_dpm_from_noise(xT, params, steps=6, order=2, guide_w=3.0)
    assert x.shape == (N, 1, H, H) and inter.shape == (6, N, 1, H, H) and np.isfinite(inter).all()
    x, inter = d.sample_dpm_from_noise(xT, None, steps=None, spacing=[2, 50, 100])
    assert x.shape == (N, 1, H, H) and inter.shape == (3, N, 1, H, H)
    assert len(d._samplers) == 4 and all(isinstance(s, cdm_amd.DPMSolverSampler) for s in d._samplers.values())
    d.sample_dpm_from_noise(xT, params, steps=6, order=2, guide_w=3.0)
    assert len(d._samplers) == 4                                 # cached by (steps, order, spacing)
    d.sample_dpm_from_noise(xT, params, steps=6, order=1, guide_w=3.0)
    assert len(d._samplers) == 5
    # the DDIM sampler of the same steps, with eta equal to the order as a number, is another entry and another class
    d.sample_ddim_from_noise(xT, params, steps=6, eta=1.0, guide_w=3.0)
    assert len(d._samplers) == 6
    assert sum(isinstance(s, cdm_amd.DDIMSampler) for s in d._samplers.values()) == 1
    d.sample_dpm_from_noise(xT, params, steps=6, order=1, guide_w=3.0)
    assert len(d._samplers) == 6
    with pytest.raises(ValueError):
        d.sample_dpm(N, H, None, params, 0.0, steps=T + 1)
    with pytest.raises(ValueError):
        d.sample_dpm(N, H, None, params, 0.0, steps=12, order=3)


def test_one_and_two_steps(model):
    """S = 1 and S = 2 run; at S = 2 both positions are first order, so order 2 equals order 1 bit for bit."""
    import cdm_amd
    d = cdm_amd.DDPM(model, T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(8))
    xT = torch.randn(N, 1, H, H, generator=torch.Generator().manual_seed(2)).cuda()
    out = {}
    for S in (1, 2):
        for order in (1, 2):
            torch.manual_seed(12)
            x, inter = d.sample_dpm_from_noise(xT, params, steps=S, order=order, guide_w=3.0)
            assert x.shape == (N, 1, H, H) and torch.isfinite(x).all() and inter.shape == (S, N, 1, H, H)
            out[S, order] = (x.cpu(), inter)
        assert torch.equal(out[S, 1][0], out[S, 2][0]) and np.array_equal(out[S, 1][1], out[S, 2][1])
    assert not torch.equal(out[1, 2][0], out[2, 2][0])


def test_functional_sampler_solver(model):
    """sample_ddpm(..., steps=12, solver="dpmpp") is DDPM.sample_dpm under the same seed; steps=None is the ancestral
    path whatever solver says, bit for bit."""
    import cdm_amd
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(8))
    for p in (params, None):
        torch.manual_seed(9)
        a = cdm_amd.sample_ddpm(model, N, H, "cuda", p, 0.0, T, steps=12, solver="dpmpp", order=2, spacing="quadratic")
        torch.manual_seed(9)
        b, _ = cdm_amd.DDPM(model, T, "cuda").sample_dpm(N, H, None, p, 0.0, steps=12, order=2, spacing="quadratic")
        assert a.shape == (N, 1, H, H) and torch.equal(a, b)
    torch.manual_seed(9)
    a = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T, steps=12, solver="dpmpp", spacing="quadratic")
    torch.manual_seed(9)
    c = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T, steps=12, spacing="quadratic")     # solver="ddim"
    assert not torch.equal(a, c)
    with pytest.raises(ValueError):
        cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T, steps=12, solver="euler")
    T_ = 12
    torch.manual_seed(10)
    a = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T_, steps=None, solver="dpmpp")
    torch.manual_seed(10)
    b = cdm_amd.sample_ddpm(model, N, H, "cuda", params, 0.0, T_)
    assert torch.equal(a, b)


def test_in_channels_raise():
    import cdm_amd
    m = cdm_amd.ContextUnet(3, NF, NCF, H).cuda()
    d = cdm_amd.DDPM(m, 10, "cuda")
    with pytest.raises(NotImplementedError):
        d.sample_dpm(2, H, "cuda", torch.zeros(2, NCF).cuda(), 0.0, steps=5)
    with pytest.raises(NotImplementedError):
        d.sample_dpm_from_noise(torch.zeros(2, 3, H, H).cuda(), None, steps=5)


# ---------------------------------------------------------------------------------------------------------------
# 6. CLI
# ---------------------------------------------------------------------------------------------------------------
CLI_ARGS = ["1e-3", "1", "20", "6", "--synthetic", "150", "--n-feat", "16", "--batch-size", "16", "--n-samples", "3"]


def test_cli_sampler_dpmpp(tmp_path):
    r = subprocess.run([sys.executable, CLI, *CLI_ARGS, "--out-root", str(tmp_path), "--sample-steps", "5",
                        "--sampler", "dpmpp"], capture_output=True, text=True, timeout=600)
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
    assert len(lines) == 2 and all("T=20, steps=5, dpmpp order=2:" in ln for ln in lines), log
    assert "eta=" not in log


def test_cli_sampler_dpmpp_argument_errors(tmp_path):
    """--sampler dpmpp with a non-zero --eta, or without --sample-steps, is an argument error (exit status 2, before any
    output directory is made)."""
    for extra in (["--sample-steps", "5", "--sampler", "dpmpp", "--eta", "0.5"], ["--sampler", "dpmpp"]):
        r = subprocess.run([sys.executable, CLI, *CLI_ARGS, "--out-root", str(tmp_path), *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-2000:])
        assert "--sampler dpmpp" in r.stderr
        assert os.listdir(tmp_path) == []
