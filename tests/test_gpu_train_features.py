"""Training for guided sampling: context dropout, EMA weights and resumable trainer state.

  * cdm_adam_ema == cdm_adam bit for bit on p, m, v, state (the EMA rides in the same pass), sizes around one block
    and one full grid-stride pass (16384 x 256 threads) plus a tail.
  * EMA values against an fp64 EMA of the device's own parameters.  Bound: a step rounds p - ema once and the fma once
    (each at most 2^-24 relative to a value no larger than 2 max(|p|, |ema|) resp. max(|p|, |ema|)), the decay held as
    fp32 (1 - decay) adds one more 2^-24 of (1 - decay) |p - ema|, and the error carried in from earlier steps is
    multiplied by the decay (< 1): 4 * 2^-24 * max(|p|, |ema|) per step covers it, K steps add up to K times that.
  * cdm_context_drop against cdm_philox_uniform on the same stream (tests/test_gpu_rng.py holds that stream to a host
    oracle); a binomial count; p_drop = 1 on a row whose u is exactly 1.0f.
  * Trainer: the defaults and the EMA trainer walk the same trajectory; graph replay == eager with both features on;
    an injected keep mask == a default trainer on the masked context; checkpoint -> new trainer continues bit for bit;
    ema_weights() swaps and restores; sampling inside it == sampling from a model loaded with ema_state_dict().
  * the CLI flags --p-uncond / --ema / --resume, one child process per run.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
INVALID = 1          # hipErrorInvalidValue
U = 2.0 ** -24       # fp32 unit roundoff


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _adam_inputs(n, seed):
    """p with entries from 1e-6 to O(1) in magnitude (small |p| is where p - ema stops being exact), zero moments."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 1, (n,), generator=g).float()
    grads = [(torch.randn(n, generator=g) * 10.0 ** (k - 1)).cuda() for k in range(3)]
    return p.cuda(), grads


def _state(lr=1e-3):
    return torch.tensor([lr, 0.0, 0.0, 1.0], dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4_194_307])
def test_adam_ema_bit_identical_to_adam(n):
    import cdm_amd
    from cdm_amd.trainer import adam_bias_table
    L = cdm_amd.lib()
    bc = adam_bias_table(0.9, 0.999).cuda()
    p0, grads = _adam_inputs(n, seed=n)
    pa, ma, va, sa = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), _state()
    pb, mb, vb, sb = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), _state()
    ema = p0.clone()
    decay = torch.tensor([0.999], dtype=torch.float64, device="cuda")
    for k, g in enumerate(grads):
        L.cdm_adam(pa.data_ptr(), g.data_ptr(), ma.data_ptr(), va.data_ptr(), n, sa.data_ptr(), bc.data_ptr(),
                   bc.shape[0], 0.9, 0.999, 1e-8, 0.5, _s())
        L.cdm_adam_ema(pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), ema.data_ptr(), n, sb.data_ptr(),
                       bc.data_ptr(), bc.shape[0], 0.9, 0.999, 1e-8, 0.5, decay.data_ptr(), _s())
        torch.cuda.synchronize()
        for what, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb), ("state", sa, sb)):
            assert torch.equal(a, b), f"step {k}: {what} differs from cdm_adam"
    assert float(sb[1]) == 3.0
    assert not torch.equal(ema, pb) and torch.isfinite(ema).all()


def test_adam_ema_argument_checks():
    import cdm_amd
    from cdm_amd.trainer import adam_bias_table
    L = cdm_amd.lib()
    raw = L.raw("cdm_adam_ema")
    bc = adam_bias_table(0.9, 0.999).cuda()
    n = 8
    p, m, v, e = (torch.ones(n, device="cuda") for _ in range(4))
    g = torch.ones(n, device="cuda")
    st, d = _state(), torch.tensor([0.9], dtype=torch.float64, device="cuda")

    def call(n_=n, nbc=bc.shape[0], ema=e.data_ptr(), dec=d.data_ptr()):
        return raw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema, n_, st.data_ptr(), bc.data_ptr(), nbc,
                   0.9, 0.999, 1e-8, 1.0, dec, _s())
    assert call(nbc=0) == INVALID and call(n_=-1) == INVALID and call(ema=None) == INVALID and call(dec=None) == INVALID
    torch.cuda.synchronize()
    assert float(st[1]) == 0.0 and torch.equal(p, torch.ones_like(p)), "a refused call launched something"
    assert call(n_=0) == 0                      # the prep kernel alone: the step count moves, nothing else
    torch.cuda.synchronize()
    assert float(st[1]) == 1.0 and torch.equal(p, torch.ones_like(p)) and torch.equal(e, torch.ones_like(e))


def _ema_run(decays, n=100_003, graph=False):
    """K = len(decays) steps of cdm_adam_ema with decay decays[k] in step k; returns (p, ema, ema64).  graph: the
    call is captured once (after an eager first step) and replayed, the decay changed through the device double."""
    import cdm_amd
    from cdm_amd.trainer import adam_bias_table
    L = cdm_amd.lib()
    bc = adam_bias_table(0.9, 0.999).cuda()
    p, _ = _adam_inputs(n, seed=17)
    gen = torch.Generator().manual_seed(18)
    ema = (p.cpu() + 0.01 * torch.randn(n, generator=gen)).cuda()
    m, v, st = torch.zeros_like(p), torch.zeros_like(p), _state()
    g = torch.empty_like(p)
    dec = torch.zeros(1, dtype=torch.float64, device="cuda")
    ema64 = ema.double().cpu()

    def launch(stream):
        L.cdm_adam_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), n, st.data_ptr(),
                       bc.data_ptr(), bc.shape[0], 0.9, 0.999, 1e-8, 1.0, dec.data_ptr(), stream)
    cg = None
    for k, d in enumerate(decays):
        g.copy_(torch.randn(n, generator=gen) * 10.0 ** (k - 1))
        dec.fill_(d)
        if not graph or k == 0:
            launch(_s())
        elif cg is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, stream=side):
                launch(torch.cuda.current_stream().cuda_stream)
            cg.replay()
        else:
            cg.replay()
        torch.cuda.synchronize()
        p64 = p.double().cpu()
        ema64 = ema64 + (1.0 - d) * (p64 - ema64)
    return p.cpu(), ema.cpu(), ema64


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_ema_values_against_fp64(decay):
    K = 3
    p, ema, ema64 = _ema_run([decay] * K)
    err = (ema.double() - ema64).abs().max().item()
    bound = 4 * K * U * max(p.abs().max().item(), ema.abs().max().item())
    print(f"decay {decay}: max|ema - ema64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if decay == 0.0:
        assert torch.equal(ema, p)


def test_ema_decay_changes_between_graph_replays():
    """One captured cdm_adam_ema, replayed with the device double set to 0.5 and then 0.99: the EMA follows the
    fp64 EMA run with those decays, and is far from the one run with the decay of the capture throughout."""
    decays = [0.9, 0.9, 0.5, 0.99]
    p, ema, ema64 = _ema_run(decays, graph=True)
    M = max(p.abs().max().item(), ema.abs().max().item())
    err = (ema.double() - ema64).abs().max().item()
    print(f"max|ema - ema64| = {err:.3e}, bound {4 * len(decays) * U * M:.3e}")
    assert err <= 4 * len(decays) * U * M
    _, ema_fixed, _ = _ema_run([0.9] * 4, graph=True)
    assert (ema - ema_fixed).abs().max().item() > 1e-3


def _drop(c, p_drop, seed, sub, ctr, want_keep=True):
    import cdm_amd
    L = cdm_amd.lib()
    B, ncf = c.shape
    out = torch.full_like(c, float("nan"))
    keep = torch.full((B,), -1, dtype=torch.int32, device="cuda") if want_keep else None
    L.cdm_context_drop(c.data_ptr(), B, ncf, p_drop, seed, sub, ctr.data_ptr(), out.data_ptr(),
                       None if keep is None else keep.data_ptr(), _s())
    u = torch.empty(B, device="cuda")
    L.cdm_philox_uniform(u.data_ptr(), B, 0.0, 1.0, seed, sub, ctr.data_ptr(), _s())
    torch.cuda.synchronize()
    return out, keep, u


@pytest.mark.parametrize("ncf", [1, 6])
@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_context_drop_matches_the_uniform_stream(B, ncf):
    seed, sub = 0x1234_5678_9ABC, 3 << 24
    ctr = torch.tensor([7], dtype=torch.int32, device="cuda")
    c = torch.randn(B, ncf, generator=torch.Generator().manual_seed(B * 10 + ncf)).cuda()
    c0 = c.clone()
    p_drop = 0.3
    out, keep, u = _drop(c, p_drop, seed, sub, ctr)
    ref = (u >= torch.tensor(p_drop, dtype=torch.float32, device="cuda")).int()
    assert torch.equal(keep, ref)
    assert torch.equal(c, c0), "the caller's batch was written"
    k = ref.bool()
    assert torch.equal(out[k], c0[k]), "kept rows"
    assert torch.equal(out[~k].view(torch.int32), torch.zeros_like(out[~k], dtype=torch.int32)), "dropped rows are +0"
    out2, none, _ = _drop(c, p_drop, seed, sub, ctr, want_keep=False)      # keep is optional
    assert none is None and torch.equal(out2, out)
    out, keep, _ = _drop(c, 0.0, seed, sub, ctr)
    assert torch.equal(out, c0) and keep.all()
    out, keep, _ = _drop(c, 1.0, seed, sub, ctr)
    assert not out.any() and not keep.any()


@pytest.mark.parametrize("ncf", [1, 6])
def test_context_drop_p_one_drops_a_row_whose_u_is_one(ncf):
    """u01 lies in (0, 1]: element 0 of the stream (seed 0, sub 1543363) is exactly 1.0f (tests/_rng_ref.py find_u_one),
    so u < p_drop is false at p_drop = 1.  p_drop = 1 drops the row all the same; the next float below 1 is the plain
    comparison and keeps it."""
    seed, sub = 0, 1543363
    ctr = torch.tensor([0], dtype=torch.int32, device="cuda")
    c = torch.full((1, ncf), 2.5, device="cuda")
    out, keep, u = _drop(c, 1.0, seed, sub, ctr)
    assert u.view(torch.int32).item() == 0x3F800000, "the stream's first element is 1.0f"
    assert keep.tolist() == [0]
    assert torch.equal(out.view(torch.int32), torch.zeros_like(out, dtype=torch.int32)), "a +0 row"
    out, keep, _ = _drop(c, 1.0, seed, sub - 5, torch.tensor([5], dtype=torch.int32, device="cuda"))   # sub + counter
    assert keep.tolist() == [0] and not out.any()
    out, keep, _ = _drop(c, 0.99999994, seed, sub, ctr)
    assert keep.tolist() == [1] and torch.equal(out, c)


def test_context_drop_counter_and_rate():
    """The device counter selects the stream (a replayed step draws a fresh mask), and at B = 4096, p = 0.25 the
    dropped count lies within six binomial standard deviations (sqrt(4096 * 0.25 * 0.75) = 27.7) of 1024."""
    seed, sub = 42, 3 << 24
    B = 4096
    c = torch.ones(B, 6, device="cuda")
    masks = []
    for ctr in (0, 1):
        _, keep, _ = _drop(c, 0.25, seed, sub, torch.tensor([ctr], dtype=torch.int32, device="cuda"))
        masks.append(keep)
        dropped = B - int(keep.sum())
        print(f"counter {ctr}: dropped {dropped} of {B}")
        assert abs(dropped - 1024) <= 166
    assert not torch.equal(masks[0], masks[1])
    small = [_drop(c[:257], 0.3, seed, sub, torch.tensor([k], dtype=torch.int32, device="cuda"))[1] for k in (7, 8)]
    assert not torch.equal(small[0], small[1])


def test_context_drop_argument_checks():
    import cdm_amd
    raw = cdm_amd.lib().raw("cdm_context_drop")
    c = torch.ones(4, 6, device="cuda")
    out = torch.full_like(c, 5.0)

    def call(B=4, ncf=6, p=0.5, dst=None):
        return raw(c.data_ptr(), B, ncf, p, 1, 0, None, out.data_ptr() if dst is None else dst, None, _s())
    for kw in (dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(B=0), dict(ncf=0), dict(dst=c.data_ptr())):
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(c, 5.0))
    assert call() == 0


# ------------------------------------------------------------------------------------------------
# Trainer
# ------------------------------------------------------------------------------------------------
NF, B, T = 16, 4, 1500


def _model(seed=5, nf=NF):
    from cdm_amd import ContextUnet
    torch.manual_seed(seed)
    m = ContextUnet(1, nf, 6, 64).cuda().train()
    m.shortcut_source = "device"
    return m


def _batch(seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 1, 64, 64, generator=g).cuda(), torch.rand(B, 6, generator=g).cuda()


def _snap(tr):
    torch.cuda.synchronize()
    out = {"flat": tr.flat, "m": tr.m, "v": tr.v, "bn": tr.bnflat, "opt": tr.opt_state, "ctr": tr.ctr}
    if tr.ema is not None:
        out["ema"] = tr.ema
    out = {k: v.cpu().clone() for k, v in out.items()}
    out.update({"nbt." + k: v.cpu().clone() for k, v in tr.model.state_dict().items() if k.endswith("tracked")})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_ema_trainer_walks_the_default_trajectory():
    from cdm_amd import Trainer
    x, c = _batch()
    runs = []
    for kw in ({}, {"ema_decay": 0.999}):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, **kw)
        losses = [float(tr.step(x, c).item()) for _ in range(3)]
        runs.append((_snap(tr), losses, tr))
    (a, la, _), (b, lb, tr) = runs
    ema = b.pop("ema")
    _same(a, b)
    assert la == lb
    assert torch.isfinite(ema).all() and not torch.equal(ema, b["flat"]), "the EMA lags the parameters"
    with pytest.raises(RuntimeError):
        runs[0][2].ema_state_dict()
    with pytest.raises(RuntimeError):
        runs[0][2].set_ema_decay(0.5)


def test_graph_replay_equals_eager_with_both_features():
    from cdm_amd import Trainer
    x, c = _batch()
    runs = []
    for use_graph in (False, True):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=use_graph, ema_decay=0.9, p_uncond=0.5)
        losses, keeps = [], []
        for k in range(5):
            if k == 3:
                tr.set_ema_decay(0.5)
            losses.append(float(tr.step(x, c).item()))
            keeps.append(tr.cur.keep.cpu().clone())
        assert (tr.graph is not None) == use_graph
        assert torch.equal(tr.c, c), "the caller's batch was written"
        runs.append((_snap(tr), losses, torch.stack(keeps)))
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2])
    keeps = runs[1][2]
    assert 0 < int(keeps.sum()) < keeps.numel(), "20 draws at p = 0.5: some kept, some dropped"
    assert len({tuple(k.tolist()) for k in keeps}) > 1, "replays draw fresh masks"


def test_injected_keep_equals_default_trainer_on_masked_context():
    from cdm_amd import Trainer
    x, c = _batch()
    g = torch.Generator().manual_seed(6)
    inj = (torch.randn(B, 1, 64, 64, generator=g).cuda(), torch.randint(1, T + 1, (B,), generator=g).int().cuda(),
           (torch.rand(2 * NF, generator=g) * 2 - 1).cuda())
    keep = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device="cuda")
    a = Trainer(_model(), 1e-3, T, B, use_graph=False, p_uncond=0.5)
    la = float(a.step(x, c, inject=(*inj, keep)).item())
    b = Trainer(_model(), 1e-3, T, B, use_graph=False)
    lb = float(b.step(x, c * keep[:, None], inject=inj).item())
    _same(_snap(a), _snap(b))
    assert la == lb
    assert torch.equal(a.c, c)
    d = Trainer(_model(), 1e-3, T, B, use_graph=False)          # and the mask matters
    d.step(x, c, inject=inj)
    assert not torch.equal(d.flat, a.flat)


def _feature_trainer(seed_model=5, **kw):
    from cdm_amd import Trainer
    kw = {"ema_decay": 0.9, "p_uncond": 0.25, **kw}
    return Trainer(_model(seed_model), 1e-3, T, B, seed=9, **kw)


def test_checkpoint_continues_bit_identically(tmp_path):
    """The trainers run one after the other: models of one shape share an engine, and a captured step must not be
    replayed once another model's trainer has stepped on it."""
    x, c = _batch()
    tr = _feature_trainer()
    for _ in range(2):
        tr.step(x, c)
    torch.save(tr.state_dict(), tmp_path / "trainer.pt")
    tr.set_lr(5e-4)
    la = [float(tr.step(x, c).item()) for _ in range(2)]
    A = _snap(tr)
    sd = torch.load(tmp_path / "trainer.pt", weights_only=True)
    assert sd["steps"] == 2 and sd["seed"] == 9 and sd["ema_decay"] == 0.9 and sd["p_uncond"] == 0.25
    assert len(sd["model"]) == 156
    # back into the trainer that made it: its captured step survives the load
    graph = tr.graph
    assert graph is not None
    tr.load_state_dict(sd)
    assert tr.steps == 2 and float(tr.opt_state[0]) == 1e-3
    tr.set_lr(5e-4)
    lc = [float(tr.step(x, c).item()) for _ in range(2)]
    assert tr.graph is graph
    _same(A, _snap(tr))
    assert la == lc
    del tr, graph
    # a new model (other weights) and trainer
    tr2 = _feature_trainer(seed_model=77)
    tr2.load_state_dict(sd)
    assert tr2.steps == 2
    tr2.set_lr(5e-4)
    lb = [float(tr2.step(x, c).item()) for _ in range(2)]
    _same(A, _snap(tr2))
    assert la == lb


def test_checkpoint_mismatches_raise():
    from cdm_amd import Trainer
    with_ema = _feature_trainer()
    without = _feature_trainer(ema_decay=None)
    with pytest.raises(ValueError):
        without.load_state_dict(with_ema.state_dict())
    with pytest.raises(ValueError):
        with_ema.load_state_dict(without.state_dict())
    small = Trainer(_model(nf=8), 1e-3, T, B, ema_decay=0.9, p_uncond=0.25)
    with pytest.raises(ValueError):
        small.load_state_dict(with_ema.state_dict())
    bad = with_ema.state_dict()
    bad["m"] = bad["m"][:-1]
    with pytest.raises(ValueError):
        with_ema.load_state_dict(bad)


def test_ema_weights_swap_and_restore():
    x, c = _batch()
    other = _feature_trainer()          # never enters ema_weights(); run to its end before the second trainer starts
    for _ in range(2):                  # (models of one shape share an engine: see the checkpoint test)
        other.step(x, c)
    lb = float(other.step(x, c).item())
    ref = _snap(other)
    del other
    tr = _feature_trainer()
    for _ in range(2):
        tr.step(x, c)
    live = tr.flat.clone()
    ptr = tr.flat.data_ptr()
    esd = tr.ema_state_dict()
    assert len(esd) == 156
    assert any(not torch.equal(esd[n], tr.views[n]) for n in tr.views)
    with tr.ema_weights():
        msd = tr.model.state_dict()
        assert list(msd) == list(esd)
        for k in esd:
            assert torch.equal(msd[k], esd[k]), k
        with pytest.raises(RuntimeError):
            tr.step(x, c)
    assert torch.equal(tr.flat, live) and tr.flat.data_ptr() == ptr
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError("boom")
    assert torch.equal(tr.flat, live)
    la = float(tr.step(x, c).item())
    _same(_snap(tr), ref)
    assert la == lb


def test_sampling_inside_ema_weights_uses_the_ema():
    from cdm_amd import DDPM
    x, c = _batch()
    tr = _feature_trainer()
    for _ in range(3):
        tr.step(x, c)
    params = torch.rand(2, 6, generator=torch.Generator().manual_seed(3))

    def sample(model):
        model.eval()
        torch.manual_seed(5)
        out, _ = DDPM(model, 10, "cuda", z_source="host").sample_ddpm(2, 64, None, params, 0.5)
        model.train()
        return out.cpu()
    tr.model.shortcut_source = "cpu"
    live = sample(tr.model)
    with tr.ema_weights():
        inside = sample(tr.model)
    fresh = _model(seed=123)
    fresh.shortcut_source = "cpu"
    fresh.load_state_dict(tr.ema_state_dict())
    ref = sample(fresh)
    assert torch.isfinite(inside).all()
    assert torch.equal(inside, ref)
    assert not torch.equal(inside, live)
    assert torch.equal(sample(tr.model), live), "the live weights sample as before"


def _cli(args, tmp_path):
    r = subprocess.run([sys.executable, CLI, *args, "--synthetic", "150", "--n-feat", "16", "--batch-size", "16",
                        "--n-samples", "2", "--out-root", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_guidance_flags_and_resume(tmp_path):
    import numpy as np
    ck = tmp_path / "paper_lr_0.001_epochs_1_timesteps_20_params_6" / "weights" / "trainer_epoch_1.pt"
    flags = ["--p-uncond", "0.2", "--ema", "0.99", "--resume", str(ck), "--guide-w", "0.5"]
    out = _cli(["1e-3", "1", "20", "6", *flags], tmp_path)
    assert "Epoch 1/1" in out and "Resumed" not in out
    assert sorted(os.listdir(ck.parent)) == ["model_epoch_1.pth", "model_epoch_1_ema.pth", "trainer_epoch_1.pt"]
    live = torch.load(ck.parent / "model_epoch_1.pth", weights_only=True)
    ema = torch.load(ck.parent / "model_epoch_1_ema.pth", weights_only=True)
    assert list(ema) == list(live) and len(ema) == 156
    assert not torch.equal(ema["out.3.weight"], live["out.3.weight"])
    assert torch.equal(ema["init_conv.conv1.1.running_mean"], live["init_conv.conv1.1.running_mean"])
    assert np.isfinite(np.load(ck.parent.parent / "generated_samples.npy")).all()
    out = _cli(["1e-3", "2", "20", "6", *flags, "--no-sample"], tmp_path)
    assert "Resumed from" in out and "Epoch 2/2" in out and "Epoch 1/2" not in out
    run2 = tmp_path / "paper_lr_0.001_epochs_2_timesteps_20_params_6"
    loss = np.load(run2 / "loss_log.npy")
    assert loss.shape == (2,) and np.isfinite(loss).all()
    assert sorted(os.listdir(run2 / "weights")) == ["model_epoch_2.pth", "model_epoch_2_ema.pth", "trainer_epoch_2.pt"]
