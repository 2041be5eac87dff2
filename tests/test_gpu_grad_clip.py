"""Global-norm gradient clipping and the non-finite step skip: cdm_grad_sumsq / cdm_adam_clipped and the Trainer option.

Bars (derived, not measured):
  * sum of squares: an fp32 square is exact in fp64, so the device sums n exact non-negative terms; any summation order
    of n non-negative fp64 terms is within (n - 1) 2^-53 S of the exact sum, the bar is twice that rounded up:
    |S_dev - S_ref| <= n 2^-52 S_ref against math.fsum of the exact squares.  (S_dev: the block partials, added exactly.)
  * norm: the square root halves the relative error of S (n 2^-53) and rounds once, the reference's sqrt rounds once:
    |norm_dev - norm_ref| <= (n + 2) 2^-53 norm_ref; the multiplication by a power-of-two grad_scale is exact.
  * everything after the coefficient is bit-exact: the clipped Adam step equals cdm_adam / cdm_adam_ema on the gradient
    (g * 1) * coef that torch computes in fp32, and a skipped step changes no bit.
"""
import ctypes
import functools
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
INVALID = 1          # hipErrorInvalidValue
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _state(lr=1e-3):
    return torch.tensor([lr, 0.0, 0.0, 1.0], dtype=torch.float64, device="cuda")


def _f64(v):
    return torch.tensor([float(v)], dtype=torch.float64, device="cuda")


@functools.lru_cache(maxsize=None)
def _bc():
    from cdm_amd.trainer import adam_bias_table
    return adam_bias_table(0.9, 0.999).cuda()


@functools.lru_cache(maxsize=None)
def _values(n):
    """(values [n] on the host, math.fsum of their exact fp64 squares): randn * 10**uniform(-3, 3)."""
    g = torch.Generator().manual_seed(1000 + n % 997)
    v = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 6.0 - 3.0)
    return v, math.fsum((v.double() * v.double()).tolist())


def _placed(v, unaligned):
    """v on the device: an allocation of its own, or a slice starting one float past one (a 4-byte-aligned base)."""
    if not unaligned:
        return v.cuda()
    buf = torch.zeros(v.numel() + 1, device="cuda")
    out = buf[1:]
    out.copy_(v)
    assert out.data_ptr() % 16 == 4
    return out


class _Clip:
    """Buffers of one cdm_adam_clipped caller."""

    def __init__(self, p, max_norm, ema=False, lr=1e-3):
        from cdm_amd.trainer import GRAD_SUMSQ_MAX_PARTIALS
        self.p = p.cuda().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.ema = self.p.clone() if ema else None
        self.decay = _f64(0.9) if ema else None
        self.state, self.max_norm = _state(lr), _f64(max_norm)
        self.partial = torch.full((GRAD_SUMSQ_MAX_PARTIALS,), float("nan"), dtype=torch.float64, device="cuda")
        self.rec = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        self.skipped = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(self, g, n=None, gscale=1.0):
        import cdm_amd
        n = self.p.numel() if n is None else n
        cdm_amd.lib().cdm_adam_clipped(
            self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
            None if self.ema is None else self.ema.data_ptr(), n, self.state.data_ptr(), _bc().data_ptr(),
            _bc().shape[0], 0.9, 0.999, 1e-8, gscale, None if self.ema is None else self.decay.data_ptr(),
            self.max_norm.data_ptr(), self.partial.data_ptr(), self.rec.data_ptr(), self.skipped.data_ptr(), _s())
        torch.cuda.synchronize()
        return self.rec.cpu().clone()

    def tensors(self):
        out = {"p": self.p, "m": self.m, "v": self.v, "state": self.state}
        if self.ema is not None:
            out["ema"] = self.ema
        return out

    def snap(self):
        torch.cuda.synchronize()
        return {k: t.cpu().clone() for k, t in self.tensors().items()}


def _plain_adam(t, g, gscale=1.0):
    """cdm_adam / cdm_adam_ema in place on the tensors of a _Clip-shaped dict t (+ "decay")."""
    import cdm_amd
    L = cdm_amd.lib()
    n = t["p"].numel()
    if "ema" in t:
        L.cdm_adam_ema(t["p"].data_ptr(), g.data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(), n,
                       t["state"].data_ptr(), _bc().data_ptr(), _bc().shape[0], 0.9, 0.999, 1e-8, gscale,
                       t["decay"].data_ptr(), _s())
    else:
        L.cdm_adam(t["p"].data_ptr(), g.data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), n, t["state"].data_ptr(),
                   _bc().data_ptr(), _bc().shape[0], 0.9, 0.999, 1e-8, gscale, _s())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 1. the norm kernel against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 65_537, 4_194_307])
def test_sumsq_and_norm_against_fp64(n, unaligned):
    import cdm_amd
    from cdm_amd.trainer import GRAD_SUMSQ_MAX_PARTIALS
    v, S_ref = _values(n)
    g = _placed(v, unaligned)
    partial = torch.full((GRAD_SUMSQ_MAX_PARTIALS,), float("nan"), dtype=torch.float64, device="cuda")
    nb = ctypes.c_int(-1)
    cdm_amd.lib().cdm_grad_sumsq(g.data_ptr(), n, partial.data_ptr(), ctypes.byref(nb), _s())
    torch.cuda.synchronize()
    assert nb.value == min(max((n + 4095) // 4096, 1), GRAD_SUMSQ_MAX_PARTIALS)
    assert torch.isnan(partial[nb.value:]).all(), "wrote past its nb partials"
    S_dev = math.fsum(partial[:nb.value].tolist())
    err, bar = abs(S_dev - S_ref), n * 2.0 ** -52 * S_ref
    print(f"n {n} unaligned {unaligned}: nb {nb.value} |S_dev - S_ref| / S_ref = {err / S_ref:.3e}, bar {bar / S_ref:.3e}")
    assert err <= bar
    c = _Clip(torch.zeros(n), INF)
    rec = c.step(g)
    norm_ref = math.sqrt(S_ref)
    nerr, nbar = abs(float(rec[0]) - norm_ref), (n + 2) * 2.0 ** -53 * norm_ref
    print(f"   norm {float(rec[0]):.17g} ref {norm_ref:.17g} err / ref {nerr / norm_ref:.3e}, bar {nbar / norm_ref:.3e}")
    assert nerr <= nbar
    assert float(rec[1]) == 1.0 and float(rec[2]) == 0.0 and int(c.skipped) == 0 and float(c.state[1]) == 1.0
    half = _Clip(torch.zeros(n), INF).step(g, gscale=0.5)
    assert float(half[0]) == 0.5 * float(rec[0]), "grad_scale = 0.5 halves the reported norm exactly"


def test_n_zero_advances_the_step_count_only():
    c = _Clip(torch.ones(4).cuda(), 1.0, ema=True)
    before = c.snap()
    rec = c.step(torch.full((4,), 7.0, device="cuda"), n=0)
    assert rec.tolist() == [0.0, 1.0, 0.0] and int(c.skipped) == 0
    after = c.snap()
    assert float(after["state"][1]) == 1.0
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(before[k], after[k]), k


# ------------------------------------------------------------------------------------------------
# 2. determinism
# ------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    n = 4_194_307
    g = _placed(_values(n)[0], False)
    _, S_ref = _values(n)
    runs = []
    for _ in range(2):
        c = _Clip(torch.zeros(n), 0.5 * math.sqrt(S_ref))
        rec = c.step(g)
        runs.append((rec.view(torch.int64), c.partial.cpu().view(torch.int64)))
    assert torch.equal(runs[0][0], runs[1][0]), "{norm, coef, skip} differ between two runs on one buffer"
    assert torch.equal(runs[0][1], runs[1][1]), "block partials differ between two runs on one buffer"
    assert 0.0 < float(runs[0][0].view(torch.float64)[1]) < 1.0


# ------------------------------------------------------------------------------------------------
# 3. clipped Adam == Adam on the pre-scaled gradient
# ------------------------------------------------------------------------------------------------
def _adam_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 1, (n,), generator=g).float()
    grads = [(torch.randn(n, generator=g) * 10.0 ** (k - 1)).cuda() for k in range(3)]
    return p.cuda(), grads


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 1_000_003])
def test_clipped_adam_equals_adam_on_prescaled_gradient(n, ema):
    from cdm_amd.trainer import clip_coef
    p0, grads = _adam_inputs(n, seed=n)
    norm0 = float(grads[0].double().norm())
    c = _Clip(p0, 0.5 * norm0, ema=ema)            # the gradients grow tenfold per step: coef < 1 in every step
    ref = {k: t.clone() for k, t in c.tensors().items()}
    unclipped = _Clip(p0, INF, ema=ema)
    plain = {k: t.clone() for k, t in unclipped.tensors().items()}
    if ema:
        ref["decay"], plain["decay"] = _f64(0.9), _f64(0.9)
    for k, g in enumerate(grads):
        rec = c.step(g)
        coef = float(rec[1])
        assert 0.0 < coef < 1.0 and float(rec[2]) == 0.0
        assert coef == clip_coef(float(rec[0]), 0.5 * norm0)
        gs = (g * 1.0) * torch.tensor(coef, dtype=torch.float32, device="cuda")
        _plain_adam(ref, gs)
        for what, t in c.tensors().items():
            assert torch.equal(t, ref[what]), f"step {k}: {what} differs from Adam on the pre-scaled gradient"
        rec = unclipped.step(g)                    # max_norm = inf: Adam on g itself
        assert float(rec[1]) == 1.0
        _plain_adam(plain, g)
        for what, t in unclipped.tensors().items():
            assert torch.equal(t, plain[what]), f"step {k}: {what} at max_norm = inf differs from cdm_adam"
    assert float(c.state[1]) == 3.0 and int(c.skipped) == 0
    assert not torch.equal(c.p, unclipped.p)


# ------------------------------------------------------------------------------------------------
# 4. non-finite skip
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [float("nan"), INF])
def test_nonfinite_gradient_skips_the_step(bad, where):
    n = 10_001                                     # three blocks and a one-element tail
    p0, grads = _adam_inputs(n, seed=4)
    c = _Clip(p0, 1.0, ema=True)
    c.step(grads[0])
    before = c.snap()
    g = grads[1].clone()
    g[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = bad
    rec = c.step(g)
    assert float(rec[2]) == 1.0 and int(c.skipped) == 1
    after = c.snap()
    for k in before:
        assert torch.equal(before[k].view(torch.int32) if before[k].dtype == torch.float32 else before[k],
                           after[k].view(torch.int32) if after[k].dtype == torch.float32 else after[k]), k
    rec = c.step(grads[1])                         # a clean gradient proceeds
    assert float(rec[2]) == 0.0 and math.isfinite(float(rec[0])) and int(c.skipped) == 1
    assert float(c.state[1]) == float(before["state"][1]) + 1.0 == 2.0
    assert not torch.equal(c.p.cpu(), before["p"]) and torch.isfinite(c.p).all() and torch.isfinite(c.ema).all()


# ------------------------------------------------------------------------------------------------
# 5. argument checks
# ------------------------------------------------------------------------------------------------
def test_argument_checks():
    import cdm_amd
    L = cdm_amd.lib()
    raw, raw_ss = L.raw("cdm_adam_clipped"), L.raw("cdm_grad_sumsq")
    n = 8
    c = _Clip(torch.ones(n).cuda(), 1.0, ema=True)
    g = torch.ones(n + 1, device="cuda")
    ptr = {"p": c.p, "g": g, "m": c.m, "v": c.v, "ema": c.ema, "state": c.state, "bc": _bc(), "decay": c.decay,
           "max_norm": c.max_norm, "partial": c.partial, "rec": c.rec, "skipped": c.skipped}
    ptr = {k: t.data_ptr() for k, t in ptr.items()}

    def call(n_=n, nbc=_bc().shape[0], **kw):
        a = {**ptr, **kw}
        return raw(a["p"], a["g"], a["m"], a["v"], a["ema"], n_, a["state"], a["bc"], nbc, 0.9, 0.999, 1e-8, 1.0,
                   a["decay"], a["max_norm"], a["partial"], a["rec"], a["skipped"], _s())
    for k in ("p", "g", "m", "v", "state", "bc", "max_norm", "partial", "rec", "skipped"):
        assert call(**{k: None}) == INVALID, k
    assert call(n_=-1) == INVALID and call(nbc=0) == INVALID
    assert call(ema=None) == INVALID and call(decay=None) == INVALID
    assert call(g=g.data_ptr() + 2) == INVALID, "a gradient that is not 4-byte aligned"
    nb = ctypes.c_int(-1)
    assert raw_ss(g.data_ptr(), n, None, ctypes.byref(nb), _s()) == INVALID
    assert raw_ss(g.data_ptr(), -1, c.partial.data_ptr(), ctypes.byref(nb), _s()) == INVALID
    assert raw_ss(None, n, c.partial.data_ptr(), ctypes.byref(nb), _s()) == INVALID
    torch.cuda.synchronize()
    assert nb.value == -1 and float(c.state[1]) == 0.0 and torch.isnan(c.rec).all() and torch.isnan(c.partial).all()
    assert torch.equal(c.p, torch.ones_like(c.p)) and int(c.skipped) == 0, "a refused call launched something"
    assert call() == 0 and call(ema=None, decay=None) == 0          # the EMA is optional, both or neither
    assert raw_ss(g.data_ptr() + 4, n, c.partial.data_ptr(), None, _s()) == 0     # nb_out is optional
    torch.cuda.synchronize()
    assert float(c.state[1]) == 2.0 and float(c.partial[0]) == float(n)


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


def _host_norm(g):
    g = g.detach().double().cpu()
    return math.sqrt(math.fsum((g * g).tolist()))


@functools.lru_cache(maxsize=None)
def _first_norm():
    """Gradient norm of the first step of the unclipped trainer on _model() / _batch() (seed 9)."""
    from cdm_amd import Trainer
    tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=False)
    tr.step(*_batch())
    return _host_norm(tr.gflat)


def test_inf_threshold_walks_the_default_trajectory():
    from cdm_amd import Trainer
    x, c = _batch()
    runs = []
    for kw in ({}, {"clip_grad_norm": INF}):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, **kw)
        losses = [float(tr.step(x, c).item()) for _ in range(3)]
        runs.append((_snap(tr), losses, tr))
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    plain, clipped = runs[0][2], runs[1][2]
    assert clipped.graph is not None and clipped.check_skipped() == 0
    assert float(clipped.clip_rec[1]) == 1.0 and float(clipped.grad_norm) > 0.0
    with pytest.raises(RuntimeError):
        plain.set_clip_grad_norm(1.0)
    with pytest.raises(RuntimeError):
        plain.grad_norm
    assert plain.check_skipped() == 0
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            clipped.set_clip_grad_norm(bad)
        with pytest.raises(ValueError):
            Trainer(_model(), 1e-3, T, B, clip_grad_norm=bad)


def test_trainer_clips_with_the_documented_coefficient():
    from cdm_amd import Trainer
    from cdm_amd.trainer import clip_coef
    x, c = _batch()
    max_norm = 0.5 * _first_norm()
    tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=False, clip_grad_norm=max_norm)
    t = {"p": tr.flat.clone(), "m": tr.m.clone(), "v": tr.v.clone(), "state": tr.opt_state.clone()}
    tr.step(x, c)
    torch.cuda.synchronize()
    n = tr.total
    norm_ref = _host_norm(tr.gflat)
    norm_dev, coef, skip = tr.clip_rec.tolist()
    print(f"n {n}: grad_norm {norm_dev:.17g} host {norm_ref:.17g}, max_norm {max_norm:.9g}, coef {coef:.9g}")
    assert float(tr.grad_norm) == norm_dev and skip == 0.0
    assert abs(norm_dev - norm_ref) <= (n + 2) * 2.0 ** -53 * norm_ref
    want = clip_coef(norm_ref, max_norm)
    ulp = 2.0 ** (math.floor(math.log2(want)) - 23)                        # of fp32 at want
    assert 0.4 < coef < 0.6 and abs(coef - want) <= ulp                    # equal after fp32 rounding, or one ulp off
    gs = (tr.gflat * 1.0) * torch.tensor(coef, dtype=torch.float32, device="cuda")
    _plain_adam(t, gs)
    assert torch.equal(t["p"], tr.flat) and torch.equal(t["m"], tr.m) and torch.equal(t["v"], tr.v)
    assert torch.equal(t["state"], tr.opt_state)


def test_graph_replay_equals_eager_with_clipping_ema_and_dropout():
    from cdm_amd import Trainer
    from cdm_amd.trainer import clip_coef
    x, c = _batch()
    n0 = _first_norm()
    runs = []
    for use_graph in (False, True):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=use_graph, ema_decay=0.9, p_uncond=0.5,
                     clip_grad_norm=0.5 * n0)
        losses, recs = [], []
        for k in range(5):
            if k == 3:
                tr.set_clip_grad_norm(0.05 * n0)
            losses.append(float(tr.step(x, c).item()))
            recs.append(tr.clip_rec.cpu().clone())
        assert (tr.graph is not None) == use_graph
        runs.append((_snap(tr), losses, torch.stack(recs), int(tr.skipped)))
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2].view(torch.int64), runs[1][2].view(torch.int64))
    recs = runs[1][2]
    assert runs[0][3] == runs[1][3] == 0 and not recs[:, 2].any()
    assert float(recs[0, 1]) < 1.0, "the first step's norm is _first_norm(): clipped at half of it"
    # the replayed graph followed the new threshold: the coefficient of its own norm at 0.05 n0 from step 3 on
    for k in range(5):
        assert float(recs[k, 1]) == clip_coef(float(recs[k, 0]), (0.5 if k < 3 else 0.05) * n0), k
    assert float(recs[3, 1]) < 1.0


def test_trainer_skips_a_step_with_a_nan_gradient():
    from cdm_amd import Trainer
    x, c = _batch()
    tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=False, ema_decay=0.9, clip_grad_norm=INF)
    tr.step(x, c)
    before = _snap(tr)

    def poison(stage):
        if stage == "init":                        # the last stage to report: gflat[0] (stage "out") is complete
            tr.gflat[0:1].fill_(float("nan"))
    tr.stage_hook = poison
    tr.step(x, c)
    after = _snap(tr)
    for k in ("flat", "m", "v", "ema", "opt"):
        assert torch.equal(before[k], after[k]), k
    assert int(after["ctr"]) == int(before["ctr"]) + 1 and tr.steps == 2, "the Philox counter and steps advance"
    assert float(tr.clip_rec[2]) == 1.0
    assert tr.check_skipped(reset=False) == 1 and tr.check_skipped() == 1 and tr.check_skipped() == 0
    tr.stage_hook = None
    loss = float(tr.step(x, c).item())
    last = _snap(tr)
    assert math.isfinite(loss) and float(last["opt"][1]) == float(before["opt"][1]) + 1.0
    assert not torch.equal(last["flat"], before["flat"]) and torch.isfinite(last["flat"]).all()
    assert torch.isfinite(last["ema"]).all() and tr.check_skipped() == 0 and float(tr.clip_rec[2]) == 0.0


def _clipped_trainer(seed_model=5, **kw):
    from cdm_amd import Trainer
    kw = {"ema_decay": 0.9, "clip_grad_norm": 0.5 * _first_norm(), **kw}
    return Trainer(_model(seed_model), 1e-3, T, B, seed=9, **kw)


def test_checkpoint_with_clipping_continues_bit_identically(tmp_path):
    x, c = _batch()
    tr = _clipped_trainer()
    for _ in range(2):
        tr.step(x, c)
    tr.set_clip_grad_norm(0.25 * _first_norm())
    torch.save(tr.state_dict(), tmp_path / "trainer.pt")
    la = [float(tr.step(x, c).item()) for _ in range(2)]
    A, recA = _snap(tr), tr.clip_rec.cpu().clone()
    del tr
    sd = torch.load(tmp_path / "trainer.pt", weights_only=True)
    assert sd["clip_grad_norm"] == 0.25 * _first_norm() and int(sd["skipped"]) == 0
    tr2 = _clipped_trainer(seed_model=77)
    tr2.load_state_dict(sd)
    assert float(tr2.max_norm) == 0.25 * _first_norm()
    lb = [float(tr2.step(x, c).item()) for _ in range(2)]
    _same(A, _snap(tr2))
    assert la == lb and torch.equal(recA.view(torch.int64), tr2.clip_rec.cpu().view(torch.int64))
    assert float(recA[1]) < 1.0


def test_checkpoint_clipping_mismatches_raise():
    clipped = _clipped_trainer()
    plain = _clipped_trainer(clip_grad_norm=None)
    with pytest.raises(ValueError):
        plain.load_state_dict(clipped.state_dict())
    with pytest.raises(ValueError):
        clipped.load_state_dict(plain.state_dict())
    sd = plain.state_dict()
    assert sd["clip_grad_norm"] is None
    plain.load_state_dict(sd)                      # unclipped into unclipped
    for k in ("clip_grad_norm", "skipped"):        # and a checkpoint from before the option existed
        del sd[k]
    plain.load_state_dict(sd)
    with pytest.raises(ValueError):
        clipped.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------
# 11. the data-parallel path over RCCL, one rank
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_run(cdm_amd, ddp, max_norm):
    tr = cdm_amd.Trainer(_model(), 1e-3, T, B, seed=3, force_ddp=ddp, use_graph=False, clip_grad_norm=max_norm)
    assert tr.ddp == ddp
    x, c = _batch()
    losses, recs = [], []
    for _ in range(2):
        losses.append(float(tr.step(x, c).item()))
        recs.append(tr.clip_rec.cpu().clone())
    torch.cuda.synchronize()
    return {"p": tr.flat.cpu(), "g": tr.gflat.cpu(), "m": tr.m.cpu(), "v": tr.v.cpu(), "bn": tr.bnflat.cpu(),
            "loss": losses, "rec": torch.stack(recs), "skipped": int(tr.skipped)}


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    import cdm_amd
    probe = _ddp_run(cdm_amd, False, INF)          # the unclipped norm of the first step, to clip at half of it
    max_norm = 0.5 * float(probe["rec"][0, 0])
    out = {"ddp": _ddp_run(cdm_amd, True, max_norm), "plain": _ddp_run(cdm_amd, False, max_norm)}
    torch.save(out, os.path.join(outdir, "rccl_clip.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_path_with_clipping_equals_plain_trainer_single_rank(tmp_path):
    mp.spawn(_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "rccl_clip.pt")
    a, b = r["ddp"], r["plain"]
    for k in ("p", "g", "m", "v", "bn"):
        assert torch.equal(a[k], b[k]), k
    assert a["loss"] == b["loss"] and a["skipped"] == b["skipped"] == 0
    assert torch.equal(a["rec"].view(torch.int64), b["rec"].view(torch.int64))
    assert float(a["rec"][0, 1]) < 1.0, "clipping was active"


# ------------------------------------------------------------------------------------------------
# 12. CLI
# ------------------------------------------------------------------------------------------------
def test_cli_clip_grad(tmp_path):
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "20", "6", "--clip-grad", "1.0", "--no-sample", "--synthetic",
                        "150", "--n-feat", "16", "--batch-size", "16", "--out-root", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("Epoch 1/1")]
    assert len(line) == 1 and "skipped steps 0" in line[0], r.stdout
    norm = float(line[0].split("grad norm ")[1].split(",")[0])
    assert math.isfinite(norm) and norm > 0.0
    bad = subprocess.run([sys.executable, CLI, "1e-3", "1", "20", "6", "--clip-grad", "0", "--synthetic", "150"],
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "--clip-grad" in bad.stderr
