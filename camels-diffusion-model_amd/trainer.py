"""The DDPM training step (a8) on the HIP engine, single- or multi-GPU.

One step == code/train_diffusion_condition.py:216-230 (and code/train_diffusion.py:141-151):
    noise ~ N(0,1), t ~ U{1..T}, x_pert = perturb_input(x, t, noise), eps = ContextUnet(x_pert, t/T, c)
    (train-mode BatchNorm), loss = mse(eps, noise), backward, Adam(lr) step.

MI355X design:
  * parameters, gradients and Adam moments live in three flat fp32 buffers; the module's nn.Parameters
    are re-pointed to views of the flat parameter buffer (state_dict stays reference-compatible);
  * noise / timesteps / the per-forward random 1x1 shortcut come from on-device Philox keyed by a
    device step counter, so the whole step (repack -> forward -> mse -> backward -> Adam) is captured
    once in a hipGraph and replayed (single GPU);
  * optional, off by default (training for classifier-free guidance): context dropout (p_uncond: each sample's
    context is zeroed with that probability, one more Philox draw inside the step), an exponential moving average of
    the parameters kept by the fused Adam kernel (ema_decay; ema_weights() / ema_state_dict() to sample from it), and
    state_dict() / load_state_dict() that continue a run bit-identically;
  * optional, off by default: global-norm gradient clipping and a non-finite step skip (clip_grad_norm), computed on
    the device inside the captured step (see Trainer);
  * optional, off by default: symmetry augmentation (augment: a random flip / quarter turn and / or periodic shift per
    sample, drawn from Philox inside the step and folded into the perturb kernel's read of x0; see augment.py);
  * optional, off by default: a per-timestep loss weight (loss_weight: Min-SNR or a table), a loss-aware timestep draw
    (t_sampler="loss") and a per-timestep-bucket record of the raw loss (t_record), all on the device inside the
    captured step (csrc/tloss.hip; see Trainer and DESIGN §5);
  * data parallel: one process per GPU; each rank trains on its own shard of the global batch; the
    flat gradient buffer is laid out in backward-completion order and cut into stage buckets that are
    all-reduced (RCCL over xGMI) asynchronously as soon as the engine reports a stage complete, so the
    67 MB up0 gradient and everything after it overlaps the encoder's backward; BatchNorm running stats
    are broadcast from rank 0 each step (DDP broadcast_buffers semantics), batch statistics stay local
    to the rank (reference semantics at the local batch; no SyncBN in the reference).
"""
from __future__ import annotations

import contextlib
import struct
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ._lib import lib
from .augment import check_augment_ops, check_mode
from .diffusion import Schedule

STAGES: Tuple[Tuple[str, Tuple[str, ...]], ...] = (
    ("out", ("out.",)), ("up2", ("up2.",)), ("up1", ("up1.",)),
    ("up0emb", ("up0.", "timeembed", "contextembed")),
    ("down2", ("down2.",)), ("down1", ("down1.",)), ("init", ("init_conv.",)),
)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def backward_order(names: List[str]):
    """Parameter names in gradient-completion order, grouped by stage: [(stage, [names])]."""
    out, seen = [], set()
    for st, prefixes in STAGES:
        grp = [n for n in names if n.startswith(prefixes)]
        seen.update(grp)
        out.append((st, grp))
    missing = [n for n in names if n not in seen]
    if missing:
        raise AssertionError(f"parameters without a stage: {missing}")
    return out


class GradBucketer:
    """Stage-bucketed asynchronous gradient all-reduce over a flat gradient buffer.

    Device-agnostic (works with gloo on CPU tensors for tests, RCCL on MI355X)."""

    def __init__(self, gflat: torch.Tensor, ranges: Dict[str, Tuple[int, int]], group=None):
        import torch.distributed as dist
        self.dist = dist
        self.gflat, self.ranges, self.group = gflat, ranges, group
        self.world = dist.get_world_size(group)
        self.pending = []

    def stage_ready(self, stage: str):
        lo, hi = self.ranges[stage]
        if hi > lo:
            self.pending.append(self.dist.all_reduce(self.gflat[lo:hi], op=self.dist.ReduceOp.SUM,
                                                     group=self.group, async_op=True))

    def wait(self):
        for w in self.pending:
            w.wait()
        self.pending = []


class Trainer:
    def __init__(self, model, lrate: float, timesteps: int, batch_size: int, seed: int = 0,
                 use_graph: bool = True, group=None, broadcast_buffers: bool = True, force_ddp: bool = False,
                 ema_decay: Optional[float] = None, p_uncond: float = 0.0, clip_grad_norm: Optional[float] = None,
                 augment: str = "none", loss_weight=None, snr_gamma: float = 5.0, t_sampler: str = "uniform",
                 t_record: bool = False, t_buckets: int = 64, t_ema: float = 0.99, t_warmup: int = 10,
                 t_mix: float = 1e-3):
        """``force_ddp``: take the data-parallel path (stage-bucketed async all-reduce, rank-0 broadcasts, eager
        steps) even in a one-rank process group — RCCL readiness on a one-GPU box (tests/test_gpu_rccl.py).
        ``ema_decay``: keep ``self.ema``, an exponential moving average of the parameters, updated inside the fused
        Adam kernel (ema += (1 - decay) (p - ema) after every step; starts as a copy of the parameters).
        ``p_uncond``: probability with which a sample's context is replaced by the null condition c = 0 in a step
        (the condition the guided samplers evaluate; the reference never trains it).
        ``clip_grad_norm``: ``None`` (default) launches exactly the unguarded step.  A value > 0 puts
        ``torch.nn.utils.clip_grad_norm_(parameters, value)`` in front of the Adam update, on the device and inside
        the captured step: the global L2 norm of the flat gradient (fp64, deterministic: a fixed-order sum, no
        atomics), the coefficient ``clip_coef(norm, value)`` folded into the fused Adam kernel, and a skip flag.
        ``float("inf")`` never scales (the coefficient is exactly 1: the trajectory is the unguarded one) and keeps
        the norm report and the skip.  A step whose gradient holds a NaN / inf is skipped: parameters, Adam moments,
        Adam step count and EMA stay untouched, ``self.skipped`` (device int) rises by one; the Philox counter and
        ``self.steps`` still advance, so the next step draws fresh noise.  BatchNorm running statistics are NOT
        protected: the forward that overflowed has already written them.  ``self.grad_norm`` is the device fp64 norm
        of the last step's gradient before clipping; ``check_skipped()`` reads the counter (one host sync, per epoch).
        Data parallel: the norm is taken after the last all-reduce, of the summed buffer times 1 / world, the averaged
        gradient Adam sees; every rank holds identical bytes there, so every rank computes the same norm, coefficient
        and skip decision without another collective.
        ``augment``: ``"none"`` (default) launches exactly the unaugmented step.  ``"d4"``, ``"shift"`` and
        ``"d4+shift"`` train each sample of a step on a random image of itself under the symmetries of the data (a
        flip and quarter turns, a periodic roll, or both; augment.py has the definition): the ops [B, 3] come from one
        more Philox draw keyed by the step counter (``cdm_augment_draw``, sub-stream ``4 << 24``), and
        ``cdm_perturb_aug`` reads x0 through them in place of ``cdm_perturb``, both inside the captured step.  The
        noise is not transformed and the caller's batch in ``self.x0`` stays intact.  ``step(aug_ops=...)`` replaces
        the draw for one step (eager).  Data parallel: the per-rank seed already separates the ranks' draws.
        ``loss_weight``, ``t_sampler``, ``t_record`` (DESIGN §5 has the definitions): with all three at their defaults
        the step launches exactly what it launched without them.  ``loss_weight``: ``"min_snr"`` (the table
        ``min_snr_weights(schedule.ab_t, snr_gamma)``) or a 1-D array of T + 1 finite numbers >= 0 (entry 0 is ignored)
        multiplies each sample's squared error by ``w[t]``.  ``t_sampler="loss"`` draws t from a per-bucket table that
        follows the second moment of the weighted loss (Improved DDPM's sampler over ``min(t_buckets, T)`` buckets of
        timesteps, with the uniform share ``t_mix`` and the uniform draw until every bucket was seen ``t_warmup``
        times) and multiplies the sample's loss by the importance weight that keeps the objective unbiased;
        ``cdm_tsample_draw`` (sub-stream ``5 << 24``) takes ``cdm_philox_randint``'s place.  Any of the three keeps the
        record ``self.t_rec`` [NB, 3] (device fp64 per bucket: samples seen, EMA of the raw per-sample loss, EMA of
        the squared weighted loss; ``t_ema`` is the EMA's decay), read with ``t_loss_report()``.  Then
        ``cdm_mse_weighted`` takes ``cdm_mse``'s place and ``cdm_tloss_record`` follows it, inside the captured step.
        An injected ``t`` is used as given, with importance weight 1.  Data parallel: the weight and the record are
        local to the rank; ``t_sampler="loss"`` raises (the ranks' tables would diverge)."""
        self._t_w_host, self.NB = check_t_loss(loss_weight, snr_gamma, t_sampler, t_buckets, t_ema, t_warmup, t_mix,
                                               int(timesteps))
        self.t_sampler = t_sampler
        self._t_loss = t_sampler == "loss"
        self._tl = self._t_loss or loss_weight is not None or bool(t_record)
        import torch.distributed as dist
        if self._t_loss and dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1
                                                                                  or force_ddp):
            raise ValueError('t_sampler="loss" is single-process only: the ranks\' timestep tables would diverge')
        self._aug_mode = check_mode(augment)
        self.augment = augment
        if clip_grad_norm is not None:
            _check_max_norm(clip_grad_norm)
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1], got {ema_decay}")
        if not 0.0 <= float(p_uncond) <= 1.0:
            raise ValueError(f"p_uncond must lie in [0, 1], got {p_uncond}")
        self.model = model
        eng, P = model._engine_and_params()
        self.eng = eng
        dev = P["out.3.weight"].device
        self.dev = dev
        self.B, self.T = int(batch_size), int(timesteps)
        self.H, self.nf, self.ncf = model.h, model.n_feat, model.n_cfeat
        self.group = group
        self.ddp = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force_ddp)
        self.world = dist.get_world_size(group) if self.ddp else 1
        self.seed = int(seed)
        # ---- flat parameter / gradient / moment buffers in backward-completion order ----
        names = model._param_names
        order = backward_order(names)
        params = dict(model.named_parameters())
        total = sum(params[n].numel() for _, g in order for n in g)
        self.flat = torch.empty(total, device=dev)
        self.gflat = torch.zeros(total, device=dev)
        self.m = torch.zeros(total, device=dev)
        self.v = torch.zeros(total, device=dev)
        self.views: Dict[str, torch.Tensor] = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self.ranges: Dict[str, Tuple[int, int]] = {}
        self.offsets: Dict[str, int] = {}
        off = 0
        for st, grp in order:
            lo = off
            for n in grp:
                p = params[n]
                k = p.numel()
                view = self.flat[off:off + k].view_as(p)
                view.copy_(p.data)
                p.data = view
                self.views[n] = view
                self.grads[n] = self.gflat[off:off + k].view_as(p)
                self.offsets[n] = off
                off += k
            self.ranges[st] = (lo, off)
        self.total = total
        # ---- BatchNorm running stats in one flat buffer (one broadcast per step under DDP) ----
        bufs = [(n, b) for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))]
        self.bnflat = torch.empty(sum(b.numel() for _, b in bufs), device=dev)
        off = 0
        for n, b in bufs:
            mod = model.get_submodule(n.rsplit(".", 1)[0])
            view = self.bnflat[off:off + b.numel()]
            view.copy_(b)
            mod._buffers[n.rsplit(".", 1)[1]] = view
            off += b.numel()
        self.broadcast_buffers = broadcast_buffers
        if self.ddp:
            dist.broadcast(self.flat, 0, group=group)
            dist.broadcast(self.bnflat, 0, group=group)
            self.bucketer = GradBucketer(self.gflat, self.ranges, group)
        # ---- averaged weights (after the broadcast: every rank starts from rank 0's) and context dropout ----
        self.ema = self.flat.clone() if ema_decay is not None else None
        self.ema_decay = None if ema_decay is None else torch.tensor([float(ema_decay)], dtype=torch.float64, device=dev)
        self.p_uncond = float(p_uncond)
        self._in_ema = False          # inside ema_weights(): flat holds the EMA, a step would train it
        # ---- gradient clipping / step skip: device max_norm (like lr: captured steps follow it), the sum-of-squares
        #      partials, the record {norm, coef, skip} of the last step and the skipped-step counter ----
        self.clip = clip_grad_norm is not None
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.clip:
            self.max_norm = torch.tensor([float(clip_grad_norm)], dtype=torch.float64, device=dev)
            self.clip_partial = torch.zeros(GRAD_SUMSQ_MAX_PARTIALS, dtype=torch.float64, device=dev)
            self.clip_rec = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev)
        # ---- optimizer state on device (fp64, as torch keeps lr / step as Python floats):
        #      [lr, step, -step_size, sqrt(bc2)] + the host-evaluated bias-correction table ----
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.opt_state = torch.tensor([float(lrate), 0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        self.adam_bc = adam_bias_table(*self.betas).to(dev)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=dev)   # steps with a NaN / inf loss
        # ---- timestep-aware loss: the weight table [T + 1], the record [NB][3] = {n, m1, m2} and, with the loss-aware
        #      draw, its table (cdf [NB] fp64, iw_tab [NB] fp32; the uniform form until the record is warm) ----
        self.t_w = self.t_rec = self.t_cdf = self.t_iw_tab = None
        if self._tl:
            self.t_alpha, self.t_warmup, self.t_mix = 1.0 - float(t_ema), int(t_warmup), float(t_mix)
            if self._t_w_host is not None:
                self.t_w = self._t_w_host.to(dev)
            self.t_rec = torch.zeros(self.NB, 3, dtype=torch.float64, device=dev)
            if self._t_loss:
                edges = t_bucket_edges(self.T, self.NB)
                self.t_cdf = (torch.from_numpy(edges[1:]).double() / float(self.T)).to(dev)
                self.t_iw_tab = torch.ones(self.NB, device=dev)
        # ---- step buffers (per batch size: the epoch's ragged last batch gets its own) ----
        self.sched = Schedule(self.T, dev)
        self.sc = torch.empty(2 * self.nf, device=dev)
        self.nb = 256
        self.partial = torch.empty(2 * self.nb, device=dev)
        self.loss = torch.zeros(1, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bufs: Dict[int, "_StepBufs"] = {}
        self._use(self.B)
        self.use_graph = bool(use_graph) and not self.ddp
        self.graph = None
        self.steps = 0
        self._inject = None
        self._aug_ops = None          # step(aug_ops=...): this step's ops in place of the device draw
        self.stage_hook = None        # optional extra on_stage(name) callback (tests / tracing)
        self.grad_numel = None        # per-step override of the loss-mean count (data-parallel ragged batches)

    # -------------------------------------------------------------------------------------------
    def _use(self, B: int):
        b = self._bufs.get(B)
        if b is None:
            b = self._bufs[B] = _StepBufs(self.eng, B, self.H, self.ncf, self.dev, aug=self._aug_mode != 0,
                                          tl=self._tl, t_loss=self._t_loss)
        self.cur = b
        return b

    @property
    def x0(self):
        return self.cur.x0

    @property
    def c(self):
        return self.cur.c

    def P(self):
        _, P = self.model._engine_and_params()
        return P

    def set_lr(self, lr: float):
        """optim.param_groups[0]['lr'] = lr (code/train_diffusion_condition.py:213); exact Python-float lr."""
        self.opt_state[0:1].fill_(float(lr))

    def set_ema_decay(self, decay: float):
        """New EMA decay from the next step on (a device double, like lr: captured steps follow it)."""
        if self.ema is None:
            raise RuntimeError("this Trainer keeps no EMA weights (ema_decay=None)")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1], got {decay}")
        self.ema_decay.fill_(float(decay))

    def set_clip_grad_norm(self, max_norm: float):
        """New clipping threshold from the next step on (a device double, like lr: captured steps follow it)."""
        if not self.clip:
            raise RuntimeError("this Trainer does not clip gradients (clip_grad_norm=None)")
        _check_max_norm(max_norm)
        self.max_norm.fill_(float(max_norm))

    @property
    def grad_norm(self) -> torch.Tensor:
        """Device fp64 scalar: the global L2 norm of the last step's (averaged) gradient, before clipping."""
        if not self.clip:
            raise RuntimeError("this Trainer does not clip gradients (clip_grad_norm=None)")
        return self.clip_rec[0]

    def check_skipped(self, reset: bool = True) -> int:
        """Number of steps since the last check that were skipped for a NaN / inf gradient (always 0 without
        clip_grad_norm).  One host sync: call it once per epoch, not per step."""
        n = int(self.skipped.item())
        if reset and n:
            self.skipped.zero_()
        return n

    def _need_t_rec(self):
        if not self._tl:
            raise RuntimeError("this Trainer keeps no per-timestep record (loss_weight=None, t_sampler='uniform', "
                               "t_record=False)")

    def set_t_options(self, t_ema: Optional[float] = None, t_warmup: Optional[int] = None,
                      t_mix: Optional[float] = None):
        """New record decay / warm-up count / uniform share from the next step on.  They are plain launch arguments of
        ``cdm_tloss_record``: the captured step is dropped and captured again."""
        self._need_t_rec()
        check_t_loss(None, 1.0, "uniform", 1, 1.0 - self.t_alpha if t_ema is None else t_ema,
                     self.t_warmup if t_warmup is None else t_warmup, self.t_mix if t_mix is None else t_mix, 1)
        if t_ema is not None:
            self.t_alpha = 1.0 - float(t_ema)
        if t_warmup is not None:
            self.t_warmup = int(t_warmup)
        if t_mix is not None:
            self.t_mix = float(t_mix)
        self.graph = None

    def t_loss_report(self) -> Dict[str, np.ndarray]:
        """The per-bucket record as host arrays: ``edges`` [NB + 1] (bucket k holds the timesteps edges[k] + 1 ..
        edges[k + 1]), ``count`` [NB] (samples seen), ``ema_loss`` [NB] (EMA of the raw per-sample loss; 0 where
        count is 0) and ``prob`` [NB] (the probability the next draw gives the bucket: q_k of the loss-aware table, or
        n_k / T with the uniform draw).  One host sync: call it once per epoch, not per step."""
        self._need_t_rec()
        rec = self.t_rec.cpu().numpy()
        edges = t_bucket_edges(self.T, self.NB)
        if self._t_loss:
            prob = t_table(rec, self.T, self.NB, self.t_warmup, self.t_mix)[2]
        else:
            prob = np.diff(edges).astype(np.float64) / float(self.T)
        return {"edges": edges, "count": rec[:, 0].astype(np.int64), "ema_loss": rec[:, 1].copy(), "prob": prob}

    def check_finite(self, reset: bool = True) -> int:
        """Number of steps since the last check whose loss was NaN / inf (SURVEY §5 failure guard).  One host sync:
        call it once per epoch, not per step."""
        n = int(self.nonfinite.item())
        if reset and n:
            self.nonfinite.zero_()
        return n

    # ---- EMA weights ---------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this Trainer keeps no EMA weights (ema_decay=None)")

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's state dict with the parameters taken from the EMA (copies).  The BatchNorm buffers are the live
        ones: running statistics are moving averages already."""
        self._need_ema()
        out = {}
        for k, v in self.model.state_dict().items():
            off = self.offsets.get(k)
            out[k] = (v.detach() if off is None else self.ema[off:off + v.numel()].view_as(v)).clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the model on the EMA weights: ``with trainer.ema_weights(): DDPM(model, T).sample_ddpm(...)``.
        The EMA is copied into the flat parameter buffer (the parameters keep their addresses, so captured steps stay
        valid) and the live parameters are put back, bit for bit, on exit.  No training step inside the block."""
        self._need_ema()
        live = self.flat.clone()
        self.flat.copy_(self.ema)
        self.eng.invalidate()
        self._in_ema = True
        try:
            yield self.model
        finally:
            self._in_ema = False
            self.flat.copy_(live)
            self.eng.invalidate()

    # ---- checkpointing -------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        """Everything a run needs to continue bit-identically (host copies): the model's state dict (parameters and
        BatchNorm buffers, num_batches_tracked included), the Adam moments and the EMA in the flat layout, the device
        optimizer state [lr, step, ...], the Philox step counter and the scalar settings the draws depend on."""
        def cpu(t):
            return t.detach().cpu().clone()
        out = {
            "version": 1,
            "model": {k: cpu(v) for k, v in self.model.state_dict().items()},
            "layout": list(self.offsets),
            "m": cpu(self.m), "v": cpu(self.v), "ema": None if self.ema is None else cpu(self.ema),
            "opt_state": cpu(self.opt_state), "ctr": cpu(self.ctr), "nonfinite": cpu(self.nonfinite),
            "steps": int(self.steps), "seed": int(self.seed),
            "ema_decay": None if self.ema is None else float(self.ema_decay.item()),
            "p_uncond": float(self.p_uncond),
            "clip_grad_norm": float(self.max_norm.item()) if self.clip else None, "skipped": cpu(self.skipped),
            "augment": self.augment,
        }
        if self._tl:               # with the options off the keys are those of a trainer from before them
            out["t_loss"] = {
                "rec": cpu(self.t_rec), "cdf": None if self.t_cdf is None else cpu(self.t_cdf),
                "iw_tab": None if self.t_iw_tab is None else cpu(self.t_iw_tab),
                "w": None if self.t_w is None else cpu(self.t_w), "t_sampler": self.t_sampler, "t_buckets": int(self.NB),
                "alpha": float(self.t_alpha), "t_warmup": int(self.t_warmup), "t_mix": float(self.t_mix),
            }
        return out

    def load_state_dict(self, sd: Dict[str, object]):
        """Continue from ``state_dict()`` output.  Every tensor is copied into the buffer the trainer already holds
        (addresses stay: a captured step survives, unless the seed or p_uncond it was captured with changes)."""
        if (sd.get("ema") is None) != (self.ema is None):
            raise ValueError("the checkpoint has EMA weights and the trainer was built with ema_decay=None"
                             if self.ema is None else
                             "the trainer keeps EMA weights and the checkpoint has none")
        if (sd.get("clip_grad_norm") is not None) != self.clip:     # checkpoints from before the option: off
            raise ValueError("the checkpoint clips gradients and the trainer was built with clip_grad_norm=None"
                             if not self.clip else
                             "the trainer clips gradients and the checkpoint was written without clipping")
        if sd.get("augment", "none") != self.augment:               # checkpoints from before the option: "none"
            raise ValueError(f"the checkpoint was written with augment={sd.get('augment', 'none')!r} and the trainer "
                             f"was built with augment={self.augment!r}")
        tl = sd.get("t_loss")                                       # checkpoints from before the option: off
        if (tl is not None) != self._tl:
            raise ValueError("the checkpoint keeps a per-timestep loss record and the trainer was built without "
                             "loss_weight, t_sampler='loss' or t_record" if not self._tl else
                             "the trainer keeps a per-timestep loss record and the checkpoint has none")
        if tl is not None:
            if tl["t_sampler"] != self.t_sampler or int(tl["t_buckets"]) != self.NB:
                raise ValueError(f"the checkpoint was written with t_sampler={tl['t_sampler']!r} over "
                                 f"{int(tl['t_buckets'])} buckets and the trainer was built with "
                                 f"t_sampler={self.t_sampler!r} over {self.NB}")
            if (tl["w"] is None) != (self.t_w is None) or \
                    (tl["w"] is not None and not torch.equal(tl["w"].cpu(), self.t_w.cpu())):
                raise ValueError("the checkpoint was written with another loss_weight than the trainer was built with")
            if tuple(tl["rec"].shape) != (self.NB, 3):
                raise ValueError("t_loss.rec: size mismatch")
        if list(sd["layout"]) != list(self.offsets):
            raise ValueError("checkpoint holds a different parameter list than this model")
        own = self.model.state_dict()
        msd = sd["model"]
        if set(msd) != set(own):
            raise ValueError("checkpoint holds a different state dict than this model")
        for k, v in own.items():
            if tuple(msd[k].shape) != tuple(v.shape):
                raise ValueError(f"{k}: checkpoint shape {tuple(msd[k].shape)}, model {tuple(v.shape)}")
        for k in ("m", "v", "ema"):
            if sd[k] is not None and sd[k].numel() != self.total:
                raise ValueError(f"{k}: checkpoint holds {sd[k].numel()} values, the trainer {self.total}")
        if tuple(sd["opt_state"].shape) != tuple(self.opt_state.shape):
            raise ValueError("opt_state: size mismatch")
        with torch.no_grad():
            for k, v in own.items():         # state_dict() tensors alias the flat buffers: in-place copies
                v.copy_(msd[k])
            self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
            if self.ema is not None:
                self.ema.copy_(sd["ema"])
                self.ema_decay.fill_(float(sd["ema_decay"]))
            self.opt_state.copy_(sd["opt_state"]); self.ctr.copy_(sd["ctr"]); self.nonfinite.copy_(sd["nonfinite"])
            if self.clip:
                self.max_norm.fill_(float(sd["clip_grad_norm"]))
            if sd.get("skipped") is not None:
                self.skipped.copy_(sd["skipped"])
            else:
                self.skipped.zero_()
            if tl is not None:
                self.t_rec.copy_(tl["rec"])
                if self._t_loss:
                    self.t_cdf.copy_(tl["cdf"]); self.t_iw_tab.copy_(tl["iw_tab"])
        if tl is not None and (float(tl["alpha"]), int(tl["t_warmup"]), float(tl["t_mix"])) != \
                (self.t_alpha, self.t_warmup, self.t_mix):
            self.t_alpha, self.t_warmup, self.t_mix = float(tl["alpha"]), int(tl["t_warmup"]), float(tl["t_mix"])
            self.graph = None                # launch arguments of the captured step
        self.steps = int(sd["steps"])
        if int(sd["seed"]) != self.seed or float(sd["p_uncond"]) != self.p_uncond:
            self.seed, self.p_uncond = int(sd["seed"]), float(sd["p_uncond"])
            self.graph = None                # both are launch arguments of the captured step
        self.eng.invalidate()

    def _body(self, s: int):
        lb = lib()
        sb = self.cur
        B, HW, nf = sb.B, self.H * self.H, self.nf
        P = self._P
        seed = self.seed * 1000003 + (self._rank() << 20)
        if self._inject is None:
            lb.cdm_philox_normal(_p(sb.noise), B * HW, seed, 0, _p(self.ctr), s)
            if self._t_loss:       # the loss-aware draw: t and its importance weight from the table of the step before
                lb.cdm_tsample_draw(_p(sb.t_int), _p(sb.iw), B, self.T, self.NB, _p(self.t_cdf), _p(self.t_iw_tab),
                                    seed, 5 << 24, _p(self.ctr), s)
            else:
                lb.cdm_philox_randint(_p(sb.t_int), B, 1, self.T, seed, 1 << 24, _p(self.ctr), s)
            lb.cdm_philox_uniform(_p(self.sc), 2 * nf, -1.0, 1.0, seed, 2 << 24, _p(self.ctr), s)
        else:                      # parity mode: caller-provided draws (eager only)
            noise, t_int, sc = self._inject[:3]
            sb.noise.copy_(noise.reshape(-1)); sb.t_int.copy_(t_int.reshape(-1))
            self.sc.copy_(sc.reshape(-1))
        c_in = sb.c
        if self.p_uncond > 0.0:    # context dropout: the engine reads c_eff, the caller's batch in sb.c stays intact
            c_in = sb.c_eff
            if self._inject is not None and len(self._inject) > 3:
                sb.keep.copy_(self._inject[3].reshape(-1))
                torch.where(sb.keep[:, None] != 0, sb.c, torch.zeros((), device=self.dev), out=sb.c_eff)
            else:
                lb.cdm_context_drop(_p(sb.c), B, self.ncf, self.p_uncond, seed, 3 << 24, _p(self.ctr), _p(sb.c_eff),
                                    _p(sb.keep), s)
        if self._aug_mode == 0:
            lb.cdm_perturb(_p(sb.x0), _p(sb.noise), _p(sb.t_int), None, 0, _p(self.sched.sab), _p(self.sched.omab), B,
                           HW, self.T, _p(sb.xpert), _p(sb.t_in), s)
        else:                      # symmetry augmentation: xpert reads x0 through the ops, sb.x0 stays intact
            if self._aug_ops is not None:
                sb.ops.copy_(self._aug_ops)
            else:
                lb.cdm_augment_draw(_p(sb.ops), B, self.H, self._aug_mode, seed, 4 << 24, _p(self.ctr), s)
            lb.cdm_perturb_aug(_p(sb.x0), _p(sb.ops), _p(sb.noise), _p(sb.t_int), None, 0, _p(self.sched.sab),
                               _p(self.sched.omab), B, HW, self.H, self.T, _p(sb.xpert), _p(sb.t_in), s)
        self.eng.repack(P, True, s)
        eps = self.eng.forward(sb.ws, P, sb.xpert, sb.t_in, c_in, self.sc[:nf], self.sc[nf:], B, s)
        gnum = float(B * HW) if self.grad_numel is None else float(self.grad_numel)
        if self._tl:               # per-row sums, the weighted loss and gradient, then the record (and the table)
            iw = sb.iw if self._t_loss and self._inject is None else None     # an injected t: importance weight 1
            lb.cdm_mse_weighted(_p(eps), _p(sb.noise), B, HW, _p(sb.t_int), _p(self.t_w), _p(iw), gnum, _p(sb.deps),
                                _p(sb.row_sq), _p(sb.row_g), _p(self.loss), _p(self.grads["out.3.bias"]),
                                _p(self.nonfinite), s)
            lb.cdm_tloss_record(_p(sb.row_sq), _p(sb.t_int), _p(self.t_w), B, HW, self.T, self.NB, self.t_alpha,
                                _p(self.t_rec), 1 if self._t_loss else 0, self.t_warmup, self.t_mix, _p(self.t_cdf),
                                _p(self.t_iw_tab), s)
        else:
            lb.cdm_mse(_p(eps), _p(sb.noise), B * HW, gnum, _p(sb.deps), _p(self.partial), self.nb, _p(self.loss),
                       _p(self.grads["out.3.bias"]), _p(self.nonfinite), s)
        hooks = [h for h in (self.bucketer.stage_ready if self.ddp else None, self.stage_hook) if h is not None]
        hook = (lambda name: [h(name) for h in hooks]) if hooks else None
        self.eng.backward(sb.ws, P, sb.deps, self.grads, s, out3_bias_done=True, on_stage=hook)
        if self.ddp:
            self.bucketer.wait()
        if self.clip:              # norm of the (summed) buffer, coefficient and skip flag, then Adam: all on device
            lb.cdm_adam_clipped(_p(self.flat), _p(self.gflat), _p(self.m), _p(self.v), _p(self.ema), self.total,
                                _p(self.opt_state), _p(self.adam_bc), self.adam_bc.shape[0], self.betas[0],
                                self.betas[1], self.eps, 1.0 / self.world, _p(self.ema_decay), _p(self.max_norm),
                                _p(self.clip_partial), _p(self.clip_rec), _p(self.skipped), s)
        elif self.ema is None:
            lb.cdm_adam(_p(self.flat), _p(self.gflat), _p(self.m), _p(self.v), self.total, _p(self.opt_state),
                        _p(self.adam_bc), self.adam_bc.shape[0], self.betas[0], self.betas[1], self.eps,
                        1.0 / self.world, s)
        else:
            lb.cdm_adam_ema(_p(self.flat), _p(self.gflat), _p(self.m), _p(self.v), _p(self.ema), self.total,
                            _p(self.opt_state), _p(self.adam_bc), self.adam_bc.shape[0], self.betas[0], self.betas[1],
                            self.eps, 1.0 / self.world, _p(self.ema_decay), s)
        lb.cdm_counter_add(_p(self.ctr), 1, s)

    def _rank(self):
        if not self.ddp:
            return 0
        import torch.distributed as dist
        return dist.get_rank(self.group)

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            self._body(torch.cuda.current_stream().cuda_stream)
        self.graph = g

    def step(self, x0: Optional[torch.Tensor] = None, c: Optional[torch.Tensor] = None, inject=None,
             global_count: Optional[int] = None, eager: bool = False,
             aug_ops: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on batch (x0 [B,1,H,H] in [0,1], c [B, n_cfeat] or None = unconditional).

        ``inject=(noise [B,1,H,H], t [B] int, shortcut [2*n_feat] = weight|bias)`` replaces the on-device
        Philox draws for this step (parity testing; runs eagerly).  With ``p_uncond > 0`` it may carry a 4th element,
        ``keep [B]`` (0 / 1), in place of the context-dropout draw: rows with keep == 0 train on c = 0.
        ``global_count`` (data parallel): the number of samples all ranks process in this step when the ranks'
        batches differ in size; the gradient is then the mean over those samples (each rank weighted by its
        sample count, F.mse_loss over the union) instead of the mean of per-rank means.
        ``aug_ops`` (a trainer built with ``augment`` other than "none"): an integer tensor [B, 3] of (g, dy, dx) per
        sample, used in place of the device draw for this step (runs eagerly, like ``inject``; ValueError for what
        ``check_augment_ops`` rejects)."""
        if self._in_ema:
            raise RuntimeError("Trainer.step inside ema_weights(): the parameters hold the EMA")
        B = self.B if x0 is None else x0.shape[0]
        if aug_ops is not None:
            if self._aug_mode == 0:
                raise ValueError('aug_ops given to a Trainer built with augment="none"')
            aug_ops = check_augment_ops(aug_ops, B, self.H)
        self._inject, self._aug_ops = inject, aug_ops
        HW = self.H * self.H
        self.grad_numel = None if global_count is None else float(global_count) * HW / self.world
        sb = self._use(B)
        if x0 is not None:
            sb.x0.copy_(x0.reshape(B, self.H, self.H))
        if c is not None:
            sb.c.copy_(c.reshape(B, self.ncf))
        self._P = self.P()
        self.eng.invalidate()                 # the fused Adam updates parameters in place
        if self.ddp and self.broadcast_buffers:
            import torch.distributed as dist
            dist.broadcast(self.bnflat, 0, group=self.group)
        if self.use_graph and inject is None and aug_ops is None and B == self.B and self.grad_numel is None \
                and not eager:
            if self.graph is None:
                self._body(_s())          # eager warm-up step (loads every kernel) then capture
                self._capture()
            else:
                self.graph.replay()
        else:
            self._body(_s())
        self.steps += 1
        return self.loss


def shard_epoch(order: torch.Tensor, batch_size: int, world: int, rank: int):
    """Data-parallel batches of one epoch for ``rank``: [(indices, global_count)], the same count of steps on
    every rank (a rank that ran an extra step would wait forever in its all-reduce).

    Global step j takes order[j*G : (j+1)*G] with G = batch_size * world (the reference's loop over one shuffled
    epoch, code/train_diffusion_condition.py:214-216, at a global batch of G) and splits it into ``world``
    contiguous near-equal parts (sizes differ by at most one).  ``global_count`` is that step's global batch size,
    passed to Trainer.step so the gradient is the mean over all its samples (each rank weighted by its sample
    count).  A last global batch with fewer samples than ranks is skipped (at most world - 1 samples of an epoch;
    the permutation differs every epoch)."""
    G = batch_size * world
    out = []
    for j in range(0, len(order), G):
        part = order[j:j + G]
        R = len(part)
        if R < world:
            break
        lo = rank * (R // world) + min(rank, R % world)
        n = R // world + (1 if rank < R % world else 0)
        out.append((part[lo:lo + n], R))
    return out


TLOSS_MAX_BUCKETS = 1024           # CDM_TLOSS_MAX_BUCKETS (include/cdm_hip.h)


def t_bucket_edges(T: int, NB: int) -> np.ndarray:
    """edges [NB + 1] int64 of the timestep buckets: edge_k = (k T) // NB; bucket k holds edge_k + 1 .. edge_{k+1}."""
    return (np.arange(NB + 1, dtype=np.int64) * int(T)) // int(NB)


def min_snr_weights(ab_t, gamma: float = 5.0) -> torch.Tensor:
    """The Min-SNR-gamma weight of the eps-prediction loss under this project's perturbation
    x_t = sqrt(ab_t) x + (1 - ab_t) noise: w_t = min(SNR_t, gamma) / SNR_t = min(1, gamma / SNR_t) with
    SNR_t = ab_t / (1 - ab_t)^2, evaluated in fp64 and rounded to fp32 once; w_0 = 0 (unused).  [T + 1] fp32, CPU."""
    if not float(gamma) > 0.0:
        raise ValueError(f"snr_gamma must be > 0, got {gamma}")
    ab = torch.as_tensor(ab_t).detach().cpu().double().numpy().reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        om = 1.0 - ab
        snr = ab / (om * om)
        w = np.minimum(1.0, float(gamma) / snr)
    w[0] = 0.0
    return torch.from_numpy(w.astype(np.float32))


def check_t_loss(loss_weight, snr_gamma, t_sampler, t_buckets, t_ema, t_warmup, t_mix, T: int):
    """Validates the timestep-loss options of Trainer (ValueError) without touching a device; returns (the weight
    table [T + 1] fp32 on the CPU or None, NB = min(t_buckets, T))."""
    if t_sampler not in ("uniform", "loss"):
        raise ValueError(f't_sampler must be "uniform" or "loss", got {t_sampler!r}')
    if not float(snr_gamma) > 0.0:
        raise ValueError(f"snr_gamma must be > 0, got {snr_gamma}")
    if int(t_buckets) != t_buckets or not 1 <= int(t_buckets) <= TLOSS_MAX_BUCKETS:
        raise ValueError(f"t_buckets must lie in 1..{TLOSS_MAX_BUCKETS}, got {t_buckets}")
    if not 0.0 <= float(t_ema) < 1.0:
        raise ValueError(f"t_ema must lie in [0, 1), got {t_ema}")
    if int(t_warmup) != t_warmup or int(t_warmup) < 1:
        raise ValueError(f"t_warmup must be an integer >= 1, got {t_warmup}")
    if not 0.0 < float(t_mix) <= 1.0:
        raise ValueError(f"t_mix must lie in (0, 1], got {t_mix}")
    w = None
    if isinstance(loss_weight, str):
        if loss_weight != "min_snr":
            raise ValueError(f'loss_weight must be None, "min_snr" or a table of T + 1 weights, got {loss_weight!r}')
        w = min_snr_weights(Schedule(T, "cpu").ab_t, snr_gamma)
    elif loss_weight is not None:
        w = torch.as_tensor(loss_weight).detach().cpu()
        if w.dim() != 1 or w.numel() != T + 1:
            raise ValueError(f"loss_weight must be 1-D with T + 1 = {T + 1} entries, got shape {tuple(w.shape)}")
        if w.is_complex() or w.dtype == torch.bool:
            raise ValueError(f"loss_weight must hold real numbers, got {w.dtype}")
        w = w.double()
        if not bool(torch.isfinite(w[1:]).all()) or bool((w[1:] < 0).any()):
            raise ValueError("loss_weight must be finite and >= 0")
        w = w.float()
        if not bool(torch.isfinite(w[1:]).all()):
            raise ValueError("loss_weight must be finite in fp32")
        w[0] = 0.0                   # entry 0 is ignored: no timestep reads it
    return w, min(int(t_buckets), int(T))


def t_table(rec: np.ndarray, T: int, NB: int, warmup: int, mix: float):
    """The loss-aware timestep table cdm_tloss_record (mode 1) builds from the record rec [NB, 3] = {n, m1, m2}, on the
    host in the same fp64 operations: (cdf [NB] fp64, iw_tab [NB] fp32, q [NB] fp64 the bucket probabilities)."""
    edges = t_bucket_edges(T, NB)
    nk = np.diff(edges).astype(np.float64)
    rec = np.asarray(rec, dtype=np.float64)
    r = np.sqrt(rec[:, 2])
    S = np.float64(0.0)
    for v in r:
        S = S + v
    if rec[:, 0].min() < warmup or not np.isfinite(S) or not S > 0.0:
        return edges[1:].astype(np.float64) / np.float64(T), np.ones(NB, np.float32), nk / np.float64(T)
    q = ((np.float64(1.0) - np.float64(mix)) * r) / S + (np.float64(mix) * nk) / np.float64(T)
    cdf = np.empty(NB, np.float64)
    run = np.float64(0.0)
    for k in range(NB):
        run = run + q[k]
        cdf[k] = run
    return cdf, (nk / (np.float64(T) * q)).astype(np.float32), q


GRAD_SUMSQ_MAX_PARTIALS = 2048     # CDM_GRAD_SUMSQ_MAX_PARTIALS (include/cdm_hip.h): doubles cdm_adam_clipped may write


def _check_max_norm(v):
    if not float(v) > 0.0:           # rejects <= 0 and NaN; inf passes
        raise ValueError(f"clip_grad_norm must be > 0 (inf: report the norm and skip non-finite steps only), got {v}")


def clip_coef(norm: float, max_norm: float) -> float:
    """The factor the clipped Adam step multiplies the gradient with, as the device computes it
    (torch.nn.utils.clip_grad_norm_'s clamp(max_norm / (total_norm + 1e-6), max=1.0), evaluated in fp64 and rounded
    to fp32 once): float32(min(1.0, max_norm / (norm + 1e-6))).  max_norm = inf gives exactly 1.0."""
    c = min(1.0, float(max_norm) / (float(norm) + 1e-6))
    return struct.unpack("f", struct.pack("f", c))[0]


def adam_bias_table(beta1: float, beta2: float, n: int = 40960) -> torch.Tensor:
    """[n, 2] fp64: 1 - beta1**step and (1 - beta2**step)**0.5 for step = 1..n, evaluated with the Python-float
    expressions of torch.optim.Adam (_single_tensor_adam), so the device step size equals torch's bit for bit.
    The last row must be exactly (1, 1): later steps reuse it (both powers are below 2^-54 by then)."""
    rows = [(1 - beta1 ** float(s), (1 - beta2 ** float(s)) ** 0.5) for s in range(1, n + 1)]
    if rows[-1] != (1.0, 1.0):
        raise ValueError("bias-correction table too short for these betas")
    return torch.tensor(rows, dtype=torch.float64)


class _StepBufs:
    """Device buffers of one training step at batch size B (engine workspace included)."""

    def __init__(self, eng, B: int, H: int, ncf: int, dev, aug: bool = False, tl: bool = False, t_loss: bool = False):
        HW = H * H
        self.B = B
        self.x0 = torch.zeros(B, H, H, device=dev)
        self.c = torch.zeros(B, ncf, device=dev)
        self.noise = torch.empty(B * HW, device=dev)
        self.t_int = torch.empty(B, dtype=torch.int32, device=dev)
        self.t_in = torch.empty(B, device=dev)
        self.xpert = torch.empty(B, H, H, device=dev)
        self.deps = torch.empty(B, H, H, device=dev)
        self.c_eff = torch.zeros(B, ncf, device=dev)                 # c after context dropout (p_uncond > 0)
        self.keep = torch.ones(B, dtype=torch.int32, device=dev)     # its mask: 0 = dropped
        if aug:
            self.ops = torch.zeros(B, 3, dtype=torch.int32, device=dev)   # (g, dy, dx) per sample (augment != "none")
        if tl:                                                       # per-row sums of the weighted MSE (timestep loss)
            self.row_sq = torch.zeros(B, dtype=torch.float64, device=dev)
            self.row_g = torch.zeros(B, dtype=torch.float64, device=dev)
        if t_loss:
            self.iw = torch.ones(B, device=dev)                      # importance weights of the loss-aware draw
        self.ws = eng.workspace(B, True)
