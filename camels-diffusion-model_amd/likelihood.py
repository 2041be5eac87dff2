"""Likelihood / ELBO evaluation of a ContextUnet on the HIP engine.

Reference functions (same names, arguments and return values):
  calculate_likelihood(model, dataloader, timesteps, device, ab_t, b_t, a_t)
      code/train_diffusion_elbo.py:108-149  (identical copy: code/train_diffusion_paper.py:142-183)
      -> mean over samples of  sum_{t=1..T} mse_t / (2 b_t),  x_t = sqrt(ab) x + (1 - ab) noise
  calculate_elbo_and_bpd(model, dataloader, timesteps, device, ab_t, b_t, a_t)
      code/train_diffusion_paper.py:77-139  -> (avg_elbo, bpd): 10 evenly spaced t, sqrt(1 - ab) noise,
      weight 0.5 b/(1 - ab) for t > 1, divided by 10; bpd = elbo / (64*64 ln 2)
  calculate_elbo_and_bpd(x, pred_noise, noise, t, b_t, a_t, ab_t, dims)
      code/train_diffusion_elbo.py:74-105   -> (elbo, bpd) of one training batch (per-sample t)
The two same-named reference functions are told apart by their first argument (a model or a tensor).

The T-step NLL loop is the same shape as the sampler: per step a prologue (device step counter ->
t/T, shortcut row), a noise draw (on-device Philox, or a row of a pre-drawn table), the perturbation,
the full eval forward and a fused per-sample weighted-MSE accumulation.  K steps are captured in one
hipGraph and replayed; one graph per batch size (the last, ragged batch gets its own).

RNG (``noise_source``): "device" = noise on device, the per-forward 1x1 shortcut from the CPU RNG in the
reference GPU run's order; "host" = noise and shortcuts from the CPU RNG interleaved exactly as the
reference's CPU run draws them (noise_t, then the model's shortcut, for t = 1..T) — the parity mode.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ._lib import lib
from .diffusion import Schedule, _capture_steps, _draw_shortcut_row, _p, _rehomed, _run_steps, _s


def _split_batch(item):
    if torch.is_tensor(item):
        return item, None
    x = item[0]
    c = item[1] if len(item) > 1 else None
    return x, c


def _pos_int(name, v, lo=1, hi=None, msg=None) -> int:
    """int(v) of an integral, non-bool ``v`` in lo..hi (hi None: no upper end); ValueError(``msg``, or "<name> must be
    a positive integer, got <v>") otherwise."""
    if isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(msg or f"{name} must be a positive integer, got {v!r}")
    return int(v)


class _ModelDriver:
    """What the evaluator, the scan and the fit share: the model's engine and parameters, the schedule, the steps per
    graph, and one run object (device buffers + step graph) per key, built as ``run_type(self, *key)``."""
    run_type = None

    def __init__(self, model, timesteps: int, steps_per_graph: int, use_graph: bool, sched_tensors):
        self.model, self.T = model, int(timesteps)
        self.eng, self.P = model._engine_and_params()
        self.dev = self.P["out.3.weight"].device
        self.sched = Schedule(self.T, self.dev, tensors=sched_tensors)
        self.K = max(1, int(steps_per_graph))
        self.use_graph = use_graph
        self._runs = {}

    def _run(self, *key):
        r = self._runs.get(key)
        if r is None:
            r = self._runs[key] = self.run_type(self, *key)
        return r

    def _rehome(self, P):
        """The parameters moved to the tensors ``P``: every captured graph holds the old addresses."""
        self.P = P
        for r in self._runs.values():
            r.graph = None

    def _repack(self):
        self.eng.repack(self.P, False, _s(), key=self.model._eval_pack_key(self.P))

    def _refresh(self):
        """Refresh the weight pack (the eval pack, unless a subclass says otherwise); drop graphs if the parameters were
        re-homed."""
        P = _rehomed(self.model, self.P)
        if P is not None:
            self._rehome(P)
        self._repack()


class _EvalRun:
    """Device state of one batch size: inputs, noise, shortcut table, accumulator, step graph."""

    def __init__(self, ev: "LikelihoodEvaluator", B: int):
        self.ev, self.B = ev, B
        m = ev.model
        dev, H, nf, ncf = ev.dev, m.h, m.n_feat, m.n_cfeat
        T = ev.T
        E = lambda *sh: torch.empty(*sh, device=dev)
        self.HW = H * H
        self.x0 = E(B, self.HW)
        self.xt = E(B, H, H)
        self.cbuf = torch.zeros(B, ncf, device=dev)
        self.has_c = False
        self.acc = torch.zeros(B, device=dev)
        self.t_cur = E(1)
        self.cur_i = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row = 2 * nf
        self.sc_table = E(T, self.row)
        self.sc_cur = E(self.row)
        host = ev.noise_source == "host"
        # host mode: noise table row (T - t) holds the draw for step t; device mode: one noise buffer
        self.noise = E(T if host else 1, B * self.HW)
        self.nstride = B * self.HW if host else 0
        self.ws = ev.eng.workspace(B, False)
        self.graph = None

    def step(self, s, mul, div, omab):
        ev, lb = self.ev, lib()
        lb.cdm_sample_prologue(_p(self.ctr), ev.T, _p(self.cur_i), _p(self.t_cur), _p(self.sc_table), self.row,
                               _p(self.sc_cur), s)
        self._body(s, mul, div, omab, self.nstride)

    def _body(self, s, mul, div, omab, nstride):
        ev, lb = self.ev, lib()
        B, HW, nf = self.B, self.HW, ev.model.n_feat
        if ev.noise_source == "device":
            lb.cdm_philox_normal(_p(self.noise), B * HW, ev.seed, 0, _p(ev.rng_ctr), s)
            lb.cdm_counter_add(_p(ev.rng_ctr), 1, s)
        lb.cdm_perturb(_p(self.x0), _p(self.noise), None, _p(self.cur_i), nstride, _p(ev.sched.sab), _p(omab),
                       B, HW, ev.T, _p(self.xt), None, s)
        eps = ev.eng.forward(self.ws, ev.P, self.xt, self.t_cur, self.cbuf if self.has_c else None,
                             self.sc_cur[:nf], self.sc_cur[nf:], B, s)
        if mul is not None:
            lb.cdm_mse_accum(_p(eps), _p(self.noise), nstride, ev.T, B, HW, None, _p(self.cur_i), _p(mul),
                             _p(div), _p(self.acc), s)

    def capture(self, K: int):
        ev = self.ev
        rng = ev.rng_ctr.clone()

        def warm_up(s):
            self.ctr.fill_(ev.T)
            self.step(s, None, None, ev.sched.omab)                 # every kernel resident
            ev.rng_ctr.copy_(rng)                                   # ... without consuming a noise stream
        self.graph = _capture_steps(warm_up, lambda s: self.step(s, ev.nll_mul, ev.nll_div, ev.sched.omab), K)

    def load(self, x, c):
        B, dev = self.B, self.ev.dev
        self.x0.copy_(x.to(dev, torch.float32).reshape(B, self.HW))
        if self.has_c != (c is not None):
            self.graph = None                      # the captured forward reads (or skips) the context buffer
        self.has_c = c is not None
        if c is not None:
            self.cbuf.copy_(c.to(dev, torch.float32).reshape(B, -1))
        self.acc.zero_()


class LikelihoodEvaluator(_ModelDriver):
    """Holds the schedule tables, the per-batch-size runs and graphs of one model."""
    run_type = _EvalRun

    def __init__(self, model, timesteps: int, noise_source: str = "device", steps_per_graph: int = 10,
                 seed: int = 4321, use_graph: bool = True, sched_tensors=None):
        """``sched_tensors=(b_t, a_t, ab_t)``: the caller's schedule (the reference functions take them as
        arguments and use them as given); None builds the default schedule of the training scripts."""
        assert noise_source in ("device", "host")
        super().__init__(model, timesteps, steps_per_graph, use_graph, sched_tensors)
        self.noise_source = noise_source
        self.seed = seed
        self.rng_ctr = torch.zeros(1, dtype=torch.int32, device=self.dev)
        b, _, ab = (v.cpu() for v in self.sched.tensors())
        # reference fp32 expressions, evaluated once into per-step tables
        self.nll_mul = torch.ones(self.T + 1, device=self.dev)
        self.nll_div = (2 * b).to(self.dev)                                   # elbo.py:140
        self.elbo_mul = (0.5 * (b / (1.0 - ab))).to(self.dev)                # paper.py:122
        self.elbo_div = torch.full((self.T + 1,), 10.0, device=self.dev)     # paper.py:124
        self.sqrt_omab = torch.sqrt(1 - ab).to(self.dev)                     # paper.py:112

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def batch_nll(self, x, c=None) -> torch.Tensor:
        """sum_t mse_t / (2 b_t) per sample (device tensor [B]) — one batch of calculate_likelihood."""
        self._refresh()
        T, B = self.T, x.shape[0]
        r = self._run(B)
        r.load(x, c)
        rows = torch.empty(T, r.row)
        host = self.noise_source == "host"
        if host:
            zs = torch.empty(T, B * r.HW)
        for t in range(1, T + 1):                       # reference order: noise_t, then the model's shortcut
            if host:
                zs[T - t] = torch.randn(x.shape).reshape(-1)
            rows[T - t] = _draw_shortcut_row(self.model.n_feat)
        r.sc_table.copy_(rows)
        if host:
            r.noise.copy_(zs)
        if self.use_graph and r.graph is None and T >= self.K:
            r.capture(self.K)
            r.acc.zero_()
        r.ctr.fill_(T)
        _run_steps(r.graph, lambda s: r.step(s, self.nll_mul, self.nll_div, self.sched.omab), self.K, T)
        return r.acc

    @torch.no_grad()
    def batch_elbo(self, x, c=None) -> torch.Tensor:
        """Per-sample ELBO of code/train_diffusion_paper.py:104-125 (device tensor [B])."""
        self._refresh()
        T, B = self.T, x.shape[0]
        r = self._run(B)
        r.load(x, c)
        host = self.noise_source == "host"
        s = _s()
        for t in torch.linspace(1, T, 10).long():
            ti = int(t)
            if host:
                r.noise[0].copy_(torch.randn(x.shape).reshape(-1))
            r.sc_cur.copy_(_draw_shortcut_row(self.model.n_feat))
            r.cur_i.fill_(ti)
            r.t_cur.fill_(float(t / T))                # torch.tensor([t / timesteps]) with a tensor t (fp32 divide)
            r._body(s, self.elbo_mul if ti > 1 else None, self.elbo_div, self.sqrt_omab, 0)   # noise row 0
        return r.acc

    def _loop(self, dataloader, fn):
        self.model.eval()                                # the reference leaves the model in eval mode
        total, count = 0.0, 0
        for item in dataloader:
            x, c = _split_batch(item)
            total += fn(x, c).sum().item()
            count += x.shape[0]
        return total, count

    def likelihood(self, dataloader) -> float:
        total, count = self._loop(dataloader, self.batch_nll)
        return total / count

    def elbo_and_bpd(self, dataloader):
        total, count = self._loop(dataloader, self.batch_elbo)
        avg = total / count
        return avg, avg / (64 * 64 * math.log(2))


def _sched_tensors(timesteps, ab_t, b_t, a_t):
    """The caller's schedule as (b_t, a_t, ab_t) fp32 host tensors, or None for the default one.  The reference
    reads ab_t (and b_t) exactly as passed (code/train_diffusion_elbo.py:130,140; code/train_diffusion_paper.py:
    111,122); a missing a_t (unused by both estimators) is derived as 1 - b_t."""
    if ab_t is None and b_t is None and a_t is None:
        return None
    if ab_t is None or b_t is None:
        raise ValueError("pass ab_t and b_t (the tensors the estimators read) or none of the schedule tensors")
    b = torch.as_tensor(b_t).detach().to("cpu", torch.float32).reshape(-1)
    a = (1 - b) if a_t is None else torch.as_tensor(a_t).detach().to("cpu", torch.float32).reshape(-1)
    ab = torch.as_tensor(ab_t).detach().to("cpu", torch.float32).reshape(-1)
    # the reference only indexes [t] for t <= timesteps, so a longer schedule (e.g. built for a larger T) works there
    # too: its first timesteps + 1 entries are the ones read
    n = int(timesteps) + 1
    if min(b.numel(), a.numel(), ab.numel()) < n:
        raise ValueError(f"schedule tensors need at least timesteps + 1 = {n} entries")
    return b[:n].contiguous(), a[:n].contiguous(), ab[:n].contiguous()


def _cached(model, slot: str, key, build):
    """The driver ``build()`` of one ``key`` = (timesteps, noise source or steps per graph, schedule tensors or None),
    kept in the dict ``model.<slot>`` so that its graphs outlive the call."""
    cache = model.__dict__.setdefault(slot, {})
    T, opt, sched = key
    key = (int(T), opt, None if sched is None else tuple(v.numpy().tobytes() for v in sched))
    drv = cache.get(key)
    if drv is None:
        drv = cache[key] = build()
    return drv


def _evaluator(model, timesteps, noise_source, sched) -> LikelihoodEvaluator:
    return _cached(model, "_cdm_lik_eval", (timesteps, noise_source, sched),
                   lambda: LikelihoodEvaluator(model, timesteps, noise_source, sched_tensors=sched))


def calculate_likelihood(model, dataloader, timesteps, device=None, ab_t=None, b_t=None, a_t=None,
                         noise_source: str = "device") -> float:
    """code/train_diffusion_elbo.py:108-149 — mean negative log likelihood (the reference's approximation), under
    the caller's schedule ab_t / b_t when given."""
    sched = _sched_tensors(timesteps, ab_t, b_t, a_t)
    return _evaluator(model, timesteps, noise_source, sched).likelihood(dataloader)


def calculate_elbo_and_bpd_batch(x, pred_noise, noise, t, b_t, a_t, ab_t, dims):
    """code/train_diffusion_elbo.py:74-105 — (elbo, bpd) device scalars for one batch, per-sample t."""
    pred_noise = pred_noise.contiguous(); noise = noise.contiguous()
    B = pred_noise.shape[0]
    HW = pred_noise[0].numel()
    dev = pred_noise.device
    ab = ab_t.to(dev, torch.float32)
    w = (0.5 * (1.0 / (1.0 - ab) - 1.0)).contiguous()
    one = torch.ones_like(w)
    ti = torch.as_tensor(t, device=dev).reshape(-1).to(torch.int32).contiguous()
    acc = torch.zeros(B, device=dev)
    lib().cdm_mse_accum(_p(pred_noise), _p(noise), 0, ab.numel() - 1, B, HW, _p(ti), None, _p(w), _p(one), _p(acc),
                        _s())
    elbo = acc.mean()
    return elbo, elbo / (dims * math.log(2))


def calculate_elbo_and_bpd_dataset(model, dataloader, timesteps, device=None, ab_t=None, b_t=None, a_t=None,
                                   noise_source: str = "device"):
    """code/train_diffusion_paper.py:77-139 — (avg_elbo, bpd) over a dataset, under the caller's schedule when
    given."""
    sched = _sched_tensors(timesteps, ab_t, b_t, a_t)
    return _evaluator(model, timesteps, noise_source, sched).elbo_and_bpd(dataloader)


# ----------------------------------------------------------------------------------------------------------------------
# Parameter scan: which conditioning parameters does the model prefer for a map?  (not in the reference)
# ----------------------------------------------------------------------------------------------------------------------
SCAN_WEIGHTS = ("uniform", "nll")


def param_grid(base, axes) -> torch.Tensor:
    """The Cartesian grid of candidate parameter vectors [K, ncf] (fp32) over the columns named by ``axes``
    ({column index: (lo, hi, n)}: n evenly spaced values lo..hi, both ends included), every other column held at
    ``base`` [ncf].  Rows are ordered with the last axis of ``axes`` (in the dict's order) varying fastest.  Pure host
    function.  ValueError: a column outside base, n < 1, a spec that is not (lo, hi, n)."""
    b = np.asarray(torch.as_tensor(base).detach().cpu().numpy() if torch.is_tensor(base) else base,
                   dtype=np.float64).reshape(-1)
    cols, lins = [], []
    for col, spec in dict(axes).items():
        cols.append(_pos_int("axis", col, 0, b.size - 1, f"axis {col!r} is not a column of the {b.size} parameters"))
        try:
            lo, hi, n = spec
        except (TypeError, ValueError):
            raise ValueError(f"axis {col}: expected (lo, hi, n), got {spec!r}") from None
        lins.append(np.linspace(float(lo), float(hi), _pos_int(f"axis {col}: n", n)))
    grid = np.tile(b, (int(np.prod([v.size for v in lins], dtype=np.int64)) if lins else 1, 1))
    if lins:
        mesh = np.meshgrid(*lins, indexing="ij")
        for col, v in zip(cols, mesh):
            grid[:, col] = v.reshape(-1)
    return torch.from_numpy(grid.astype(np.float32))


class _Result:
    """What a scan's and a fit's result share: ``score`` [M, K] fp64 (lower is better) and the call's positions."""

    def __init__(self, score, t_grid, n_noise: int, weight: str):
        self.score = score
        self.t_grid = [int(t) for t in t_grid]
        self.n_noise, self.weight = int(n_noise), weight

    def best_index(self) -> torch.Tensor:
        return self.score.argmin(dim=1)


class ScanResult(_Result):
    """What :func:`param_scan` returns.  ``score`` [M, K] fp64 (on the device the scan ran on; lower is better),
    ``candidates`` [K, ncf] fp32 (host), ``t_grid`` (list of ints), ``n_noise`` and ``weight`` as the call had them.

    The score is a ranking statistic, not a calibrated log-likelihood (under the reference's (1 - ab) noise factor no
    weight makes it an ELBO), so the methods that turn it into weights take a ``scale`` the caller must
    choose — there is no default that would mean something.  Plain tensor code: works on any device, no kernels."""

    def __init__(self, score, candidates, t_grid, n_noise: int = 1, weight: str = "uniform"):
        super().__init__(score, t_grid, n_noise, weight)
        self.candidates = candidates

    @classmethod
    def from_logp(cls, logp, candidates) -> "ScanResult":
        """A result whose score is ``-logp`` [M, K] (fp64), ``logp[m, k]`` the log-density of map m under candidate k
        as ``DDPM.log_likelihood`` gives it (one call per candidate, the same ``seed`` so the probes are shared).
        This is the case where ``scale = 1`` means something: ``log_weights(1)`` is then log p up to a constant per
        map and ``posterior(1)`` the posterior under a flat prior over the candidates, of the discretised,
        probe-estimated density that log_likelihood documents.  ``t_grid`` is empty and ``weight`` is "logp".
        ValueError: logp not [M, K], candidates not [K, ncf], or a NaN in logp (an invalid row has no density)."""
        lp = torch.as_tensor(logp).detach().to(torch.float64)
        c = torch.as_tensor(candidates).detach().to("cpu", torch.float32)
        if lp.dim() != 2 or c.dim() != 2 or lp.shape[1] != c.shape[0] or lp.shape[0] < 1 or c.shape[0] < 1:
            raise ValueError(f"logp must be [M, K] and candidates [K, ncf], got {tuple(lp.shape)} and {tuple(c.shape)}")
        if bool(torch.isnan(lp).any()):
            raise ValueError("logp holds a NaN: an invalid row has no density to weigh")
        return cls(-lp, c, [], 1, "logp")

    def log_weights(self, scale) -> torch.Tensor:
        """-scale (score - min_k score) [M, K]: 0 at each map's best candidate."""
        s = self.score
        return -float(scale) * (s - s.min(dim=1, keepdim=True).values)

    def posterior(self, scale):
        """(mean [M, ncf], std [M, ncf], weights [M, K]): weights = softmax_k of :meth:`log_weights`, then the weighted
        mean and standard deviation of the candidates under them (fp64)."""
        w = torch.softmax(self.log_weights(scale), dim=1)
        c = self.candidates.to(w.device, w.dtype)
        mean = w @ c
        d = c[None] - mean[:, None]
        std = (w[:, :, None] * d * d).sum(1).sqrt()
        return mean, std, w

    def best(self) -> torch.Tensor:
        """The candidate with the lowest score, per map [M, ncf]."""
        return self.candidates[self.best_index().cpu()]

    def top(self, k: int) -> torch.Tensor:
        """The k lowest-scoring candidates per map, best first [M, k, ncf] (host fp32) — the natural ``start`` of
        :func:`param_fit`.  Ties keep the candidates' order.  ValueError: k outside 1..K."""
        K = self.candidates.shape[0]
        k = _pos_int("k", k, 1, K, f"k must be in 1..{K}, got {k!r}")
        idx = torch.argsort(self.score.cpu(), dim=1, stable=True)[:, :k]
        return self.candidates[idx]


def check_scan(maps, candidates, timesteps, n_cfeat, H, t_grid=None, n_steps=32, n_noise=1, weight="uniform",
               noise=None, max_rows=256):
    """Validate and normalise the arguments of a parameter scan, on the host: -> (maps [M, H, H] fp32, candidates
    [K, ncf] fp32 host, t_grid list, noise [P, M, H, H] fp32 or None).  ValueError, nothing touched: maps not
    [M, H, H] / [M, 1, H, H]; candidates not [K, n_cfeat]; a t_grid entry outside 1..timesteps or a t_grid that does
    not increase; n_noise < 1; an unknown weight; M > max_rows; noise not [P, M, H, H] with P = len(t_grid) n_noise."""
    T = int(timesteps)
    x = torch.as_tensor(maps).detach()
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3 or tuple(x.shape[1:]) != (H, H) or x.shape[0] < 1:
        raise ValueError(f"maps have shape {tuple(torch.as_tensor(maps).shape)}: expected [M, {H}, {H}] or [M, 1, {H}, {H}]")
    M = x.shape[0]
    c = torch.as_tensor(candidates).detach()
    if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != n_cfeat:
        raise ValueError(f"candidates have shape {tuple(c.shape)}: expected [K, n_cfeat = {n_cfeat}]")
    if weight not in SCAN_WEIGHTS:
        raise ValueError(f"weight must be one of {SCAN_WEIGHTS}, got {weight!r}")
    _pos_int("n_noise", n_noise)
    if t_grid is None:
        from .diffusion import timestep_subsequence
        tg = timestep_subsequence(T, n_steps)
    else:
        raw = [v.item() if hasattr(v, "item") else v for v in t_grid]
        if not raw or any(isinstance(v, bool) or int(v) != v for v in raw):
            raise ValueError("t_grid must be a non-empty list of integer timesteps")
        tg = [int(v) for v in raw]
        if any(t < 1 or t > T for t in tg):
            raise ValueError(f"t_grid must lie in 1..timesteps = {T}, got {tg}")
        if any(b <= a for a, b in zip(tg, tg[1:])):
            raise ValueError("t_grid must be strictly increasing")
    if int(max_rows) < 1 or M > int(max_rows):
        raise ValueError(f"{M} maps exceed max_rows = {max_rows}: one forward holds every map at least once")
    P = len(tg) * int(n_noise)
    z = None
    if noise is not None:
        z = torch.as_tensor(noise).detach()
        if tuple(z.shape) != (P, M, H, H):
            raise ValueError(f"noise has shape {tuple(z.shape)}: expected [P = {P}, M = {M}, {H}, {H}]")
        z = z.to(torch.float32)
    return x.to(torch.float32), c.to("cpu", torch.float32).contiguous(), tg, z


class _PositionRun:
    """Device state of one chunk shape (M maps x Kc rows per map, npos positions) and the walk over the positions that
    the scan and the fit share: inputs, noise, tables, the fp64 score accumulator, the step graph.  A subclass supplies
    ``_workspace()``, ``_score(s)`` (what follows the perturbation in a step), ``_cleared()`` and its own state."""

    def __init__(self, drv: "_PositionDriver", M: int, Kc: int, npos: int, table: bool):
        self.drv, self.M, self.Kc, self.npos = drv, M, Kc, npos
        m, dev = drv.model, drv.dev
        H, rows = m.h, M * Kc
        E = lambda *sh: torch.empty(*sh, device=dev)
        I = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        self.HW, self.rows = H * H, rows
        self.x0, self.noise = E(M, self.HW), E(M, self.HW)
        self.xt = E(rows, H, H)
        self.cbuf = torch.zeros(rows, m.n_cfeat, device=dev)
        # the captured graph holds this address, so every chunk of this shape accumulates here (ld = Kc, k0 = 0; flat
        # index m Kc + k = the batch row) and the driver copies the block into the chunk's columns of the score
        self.acc = torch.zeros(M, Kc, dtype=torch.float64, device=dev)
        self.t_cur = E(1)
        self.cur_i, self.cur_p, self.ctr, self.pos_t = I(1), I(1), I(1), I(npos)
        self.row = 2 * m.n_feat
        self.sc_table, self.sc_cur = E(npos, self.row), E(self.row)
        self.ztab = E(npos, M * self.HW) if table else None
        self.ws = self._workspace()
        self.seed = None
        self.graph = None

    def _perturbed(self, s):
        """Position ctr -> its timestep, t / T and shortcut row; its noise; x_p into ``xt``, each map Kc times."""
        d, lb = self.drv, lib()
        M, HW, T = self.M, self.HW, d.T
        lb.cdm_scan_prologue(_p(self.ctr), self.npos, T, _p(self.pos_t), _p(self.cur_i), _p(self.cur_p),
                             _p(self.t_cur), _p(self.sc_table), self.row, _p(self.sc_cur), s)
        if self.ztab is None:
            lb.cdm_philox_normal(_p(self.noise), M * HW, self.seed, 0, _p(self.cur_p), s)     # keyed by (seed, sub = p)
        else:
            lb.cdm_scan_noise_row(_p(self.ztab), _p(self.cur_p), self.npos, M * HW, _p(self.noise), s)
        lb.cdm_scan_perturb(_p(self.x0), _p(self.noise), _p(self.cur_i), _p(d.sched.sab), _p(d.sched.omab), M, self.Kc,
                            HW, T, _p(self.xt), s)

    def step(self, s):
        self._perturbed(s)
        self._score(s)

    def load(self, x, c, pos_t, rows, z, seed):
        """``c`` [M Kc, ncf]: the context of every batch row."""
        self.x0.copy_(x.to(self.drv.dev).reshape(self.M, self.HW))
        self.cbuf.copy_(c)
        self.pos_t.copy_(pos_t)
        self.sc_table.copy_(rows)
        if z is not None:
            self.ztab.copy_(z.reshape(self.npos, -1))
        if self.ztab is None and seed != self.seed:
            self.seed, self.graph = seed, None                   # the captured Philox launch holds the seed

    def positions(self):
        """One pass: every position once (graph replays, then the eager rest) on the current stream, adding into the
        accumulators as they stand.  What holds here, for both subclasses:

        * The graph is captured on first use.  The capture's warm-up launch is one real step: it advances ``ctr`` and
          adds into the accumulators, so ``_cleared()`` (every accumulator of the subclass) and ``ctr`` are zeroed
          after it, and the pass that triggered the capture starts exactly as one that found the graph ready.
        * A pass that does not capture launches its steps and nothing else.  The fit relies on it: between its passes
          ``cdm_fit_update`` clears ``acc``, ``gacc`` and ``ctr`` on the device and the host clears nothing.  The scan
          clears ``acc`` and ``ctr`` itself before every pass (:meth:`_ScanRun.run`).
        * In device-noise mode a changed seed has dropped the graph (:meth:`load`); a table-noise run never looks at
          the seed."""
        K = self.drv.K
        if self.drv.use_graph and self.graph is None and self.npos >= K:
            def warm_up(s):
                self.ctr.zero_()
                self.step(s)                                     # every kernel resident
            self.graph = _capture_steps(warm_up, self.step, K)
            for v in (*self._cleared(), self.ctr):
                v.zero_()
        _run_steps(self.graph, self.step, K, self.npos)


class _ScanRun(_PositionRun):
    """The scan's run: eval workspace; a step ends with the eval forward and ``cdm_scan_mse_accum``."""

    def _workspace(self):
        return self.drv.eng.workspace(self.rows, False)

    def _score(self, s):
        d, nf = self.drv, self.drv.model.n_feat
        eps = d.eng.forward(self.ws, d.P, self.xt, self.t_cur, self.cbuf, self.sc_cur[:nf], self.sc_cur[nf:],
                            self.rows, s)
        lib().cdm_scan_mse_accum(_p(eps), _p(self.noise), self.M, self.Kc, self.HW, _p(self.cur_i), _p(d.w), d.T,
                                 _p(self.acc), self.Kc, 0, s)

    def _cleared(self):
        return (self.acc,)

    def load(self, x, c, *walk):
        super().load(x, c.to(self.drv.dev).repeat(self.M, 1), *walk)        # row m Kc + k = candidate k

    def run(self):
        self.acc.zero_()
        self.ctr.zero_()
        self.positions()


class _PositionDriver(_ModelDriver):
    """What the scan and the fit share beyond :class:`_ModelDriver`: the weight tables and the chunk loop."""

    def __init__(self, model, timesteps: int, steps_per_graph: int = 8, use_graph: bool = True, sched_tensors=None):
        super().__init__(model, timesteps, steps_per_graph, use_graph, sched_tensors)
        b = self.sched.b_t.cpu()
        self._wtab = {"uniform": torch.ones(self.T + 1),
                      "nll": (1.0 / (2.0 * b.double())).float()}          # evaluated in fp64, rounded once
        self.w = torch.ones(self.T + 1, device=self.dev)                  # the table the captured kernels read

    def _chunks(self, x, c, tg, z, R, weight, seed, max_rows, *extra):
        """The chunk loop of a scan, a fit and :meth:`ParamFit.value_and_grad` over the K = c.shape[-2] candidates or
        starts ``c`` ([K, ncf] or [M, K, ncf]): draws the shortcut rows (once, before any chunk runs), refreshes the
        pack and the weight table, then yields (columns k0 .. k0 + kc, the loaded run) for every chunk of
        Kc = max(1, max_rows // M).  ``extra``: what keys a run beyond its shape and noise mode."""
        M, K = x.shape[0], c.shape[-2]
        npos = len(tg) * R
        Kc = min(K, max(1, max_rows // M))
        pos_t = torch.tensor(tg * R, dtype=torch.int32)                   # position p = r S + s
        rows = torch.stack([_draw_shortcut_row(self.model.n_feat) for _ in range(npos)])
        self._refresh()
        self.w.copy_(self._wtab[weight])
        for k0 in range(0, K, Kc):
            kc = min(Kc, K - k0)
            r = self._run(M, kc, npos, z is not None, *extra)
            r.load(x, c[..., k0:k0 + kc, :], pos_t, rows, z, seed)
            yield slice(k0, k0 + kc), r


class ParamScan(_PositionDriver):
    """Scores maps under candidate conditioning parameters on common noise (the diffusion-classifier statistic).

    For M maps x[m], K candidates c[k] and the P = S R positions p = r S + s (timestep t_p = t_grid[s], repeat r of
    n_noise = R; S = len(t_grid)), with one standard-normal map z_p[m] and one shortcut row sc_p per position, both shared
    by all K candidates:
        x_p[m]     = sab[t_p] x[m] + omab[t_p] z_p[m]                 (perturb_input, its fp32 roundings)
        eps_p[m,k] = model.eval()(x_p[m], t_p / T, c[k])              (shortcut sc_p)
        score[m,k] = (1 / R) sum_p w[t_p] mean_pixels (eps_p[m,k] - z_p[m])^2     accumulated in fp64
    w = 1 ("uniform") or the fp32 rounding of 1 / (2 b_t) ("nll", the weight of calculate_likelihood).  Lower is better.
    Under the reference's (1 - ab) noise factor no weight makes this an exact ELBO: it is a ranking
    statistic whose differences across k have low variance because x_p, z_p and sc_p are common.

    Same structure as :class:`LikelihoodEvaluator`: a step is ``cdm_scan_prologue`` (position counter -> timestep, t / T,
    shortcut row), the noise, ``cdm_scan_perturb``, the eval forward at batch M Kc (row m Kc + k = map m, candidate k)
    and ``cdm_scan_mse_accum``; ``steps_per_graph`` steps are captured in one hipGraph and replayed, the rest run
    eagerly.  Candidates go in chunks of Kc = max(1, max_rows // M); every chunk replays all P positions with the same
    seed and shortcut table, so a candidate's score depends on its chunk only through the forward's arithmetic (h3's
    per-tensor operand scale is taken over the chunk's batch).
    Noise: ``noise=None`` draws z_p on the device, ``cdm_philox_normal`` keyed by (seed, sub = p) over the M H W
    elements — a function of seed, p, m and the pixel alone, whatever K and the chunking; ``noise=`` [P, M, H, H] (host
    or device) is used as given (the parity mode).
    Shortcuts: one ``_draw_shortcut_row`` per position, p = 0..P-1 in order, from the CPU RNG, once per call before any
    chunk runs."""

    run_type = _ScanRun

    def scan(self, maps, candidates, t_grid=None, n_steps=32, n_noise=1, weight="uniform", seed=4321, noise=None,
             max_rows=256) -> ScanResult:
        m = self.model
        checked = check_scan(maps, candidates, self.T, m.n_cfeat, m.h, t_grid, n_steps, n_noise, weight, noise,
                             max_rows)
        return self._scan(*checked, int(n_noise), weight, int(seed), int(max_rows))

    @torch.no_grad()
    def _scan(self, x, cand, tg, z, R, weight, seed, max_rows) -> ScanResult:
        score = torch.empty(x.shape[0], cand.shape[0], dtype=torch.float64, device=self.dev)
        for sl, r in self._chunks(x, cand, tg, z, R, weight, seed, max_rows):
            r.run()
            score[:, sl] = r.acc / R
        return ScanResult(score, cand, tg, R, weight)


def param_scan(model, maps, candidates, timesteps, t_grid=None, n_steps=32, n_noise=1, weight="uniform", seed=4321,
               noise=None, max_rows=256, steps_per_graph=8, ab_t=None, b_t=None) -> ScanResult:
    """Score every map under every candidate parameter vector: ``score[m, k]``, lower = preferred (:class:`ParamScan` has
    the definition).  ``maps`` [M, H, H] or [M, 1, H, H]; ``candidates`` [K, n_cfeat] (:func:`param_grid` builds a
    grid); ``t_grid``: increasing timesteps in 1..timesteps, None = ``timestep_subsequence(timesteps, n_steps)``;
    ``n_noise``: noise draws per timestep; ``weight``: "uniform" or "nll"; ``noise``: None (device Philox keyed by
    ``seed``) or a table [P, M, H, H]; ``ab_t`` / ``b_t``: the caller's schedule, as calculate_likelihood takes it.
    Costs P ceil(K / Kc) forwards of M Kc rows, P = len(t_grid) n_noise, Kc = max(1, max_rows // M).

    The raw score is returned.  Under the reference's non-standard perturbation no weight makes it an exact
    ELBO: it ranks candidates, and its differences across k are low-variance because the perturbed input, the noise and
    the shortcut draw are common to all of them.  Arguments are validated before anything touches the device or the
    CPU RNG (ValueError: :func:`check_scan`)."""
    sched = _sched_tensors(timesteps, ab_t, b_t, None)
    checked = check_scan(maps, candidates, timesteps, model.n_cfeat, model.h, t_grid, n_steps, n_noise, weight, noise,
                         max_rows)
    ps = _cached(model, "_cdm_param_scan", (timesteps, int(steps_per_graph), sched),
                 lambda: ParamScan(model, timesteps, steps_per_graph, sched_tensors=sched))
    return ps._scan(*checked, int(n_noise), weight, int(seed), int(max_rows))


# ----------------------------------------------------------------------------------------------------------------------
# Parameter fit: gradient descent on the scan score over the conditioning vector  (not in the reference)
# ----------------------------------------------------------------------------------------------------------------------
class FitResult(_Result):
    """What :func:`param_fit` returns (tensors on the device the fit ran on):
    ``params`` [M, K, ncf] fp32, the parameters with the lowest score each start visited, and ``score`` [M, K] fp64,
    that score; ``last_params`` [M, K, ncf] after the last update; ``start`` [M, K, ncf] and ``start_score`` [M, K];
    ``history_score`` / ``history_grad_norm`` [iters + 1, M, K] fp64: the score and the 2-norm of the gradient over the
    free columns at the parameters of pass n = 1..iters + 1 (the last row is the evaluation after the last update);
    ``stalled`` [M, K] int32: updates skipped because the score or gradient was not finite; ``t_grid``, ``n_noise``,
    ``weight`` as the call had them.

    The score is the scan's ranking statistic, not a calibrated log-likelihood: the fit minimises that
    statistic on one fixed draw of noise and shortcuts.  ``params`` is a point estimate — the spread across starts is
    not a posterior width and nothing here is an error bar."""

    def __init__(self, params, score, last_params, start, history_score, history_grad_norm, stalled, t_grid,
                 n_noise: int = 1, weight: str = "uniform"):
        super().__init__(score, t_grid, n_noise, weight)
        self.params, self.last_params, self.start = params, last_params, start
        self.history_score, self.history_grad_norm, self.stalled = history_score, history_grad_norm, stalled
        self.start_score = history_score[0]

    def best(self) -> torch.Tensor:
        """Per map, the parameters of its lowest-scoring start [M, ncf]."""
        idx = self.best_index()
        return self.params[torch.arange(self.params.shape[0], device=idx.device), idx]


def check_fit(maps, start, timesteps, n_cfeat, H, iters=50, lr=0.02, free=None, bounds=(0.0, 1.0), betas=(0.9, 0.999),
              eps=1e-8, t_grid=None, n_steps=32, n_noise=1, weight="uniform", noise=None, max_rows=256, in_channels=1):
    """Validate and normalise the arguments of a parameter fit, on the host: -> (maps [M, H, H] fp32, start [M, K, ncf]
    fp32 host, t_grid list, noise [P, M, H, H] fp32 or None, free mask [ncf] int32, lo [ncf] fp64, hi [ncf] fp64).
    ValueError, nothing touched (neither the device nor the CPU RNG): in_channels > 1; start not [ncf], [K, ncf] or
    [M, K, ncf]; whatever :func:`check_scan` rejects about maps, t_grid, n_noise, weight, noise and max_rows; iters < 1;
    lr not finite or not > 0; a beta outside [0, 1); eps not finite or < 0; a free column out of range or listed twice,
    or no free column; bounds not a pair of scalars or [ncf] vectors, or lo > hi; a start value outside its bounds
    (it is not clamped)."""
    if int(in_channels) != 1:
        raise ValueError("the parameter fit is single-channel, like the samplers and the likelihood (in_channels = 1)")
    ncf = int(n_cfeat)
    s = torch.as_tensor(start).detach()
    if s.dim() not in (1, 2, 3) or s.shape[-1] != ncf or s.numel() == 0:
        raise ValueError(f"start has shape {tuple(s.shape)}: expected [{ncf}], [K, {ncf}] or [M, K, {ncf}]")
    x, flat, tg, z = check_scan(maps, s.reshape(-1, ncf), timesteps, ncf, H, t_grid, n_steps, n_noise, weight, noise,
                                max_rows)
    M = x.shape[0]
    if s.dim() == 3 and s.shape[0] != M:
        raise ValueError(f"start has shape {tuple(s.shape)}: its first axis must be the {M} maps")
    st = flat.reshape(s.shape) if s.dim() == 3 else flat.reshape(-1, ncf)[None].expand(M, -1, -1)
    st = st.contiguous()
    _pos_int("iters", iters)
    if not (math.isfinite(float(lr)) and float(lr) > 0):
        raise ValueError(f"lr must be finite and > 0, got {lr!r}")
    try:
        b1, b2 = (float(b) for b in betas)
    except (TypeError, ValueError):
        raise ValueError(f"betas must be a pair, got {betas!r}") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
    if not (math.isfinite(float(eps)) and float(eps) >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps!r}")
    cols = list(range(ncf)) if free is None else [v.item() if hasattr(v, "item") else v for v in free]
    cols = [_pos_int("free", j, 0, ncf - 1, f"free columns must lie in 0..{ncf - 1}, got {cols}") for j in cols]
    if len(set(cols)) != len(cols) or not cols:
        raise ValueError(f"free must name at least one column and none twice, got {cols}")
    mask = torch.zeros(ncf, dtype=torch.int32)
    mask[cols] = 1
    try:
        lo, hi = bounds
        lo, hi = (torch.as_tensor(b, dtype=torch.float64).detach().cpu() for b in (lo, hi))
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be a pair (lo, hi) of scalars or [{ncf}] vectors") from None
    if any(b.dim() > 1 or b.numel() not in (1, ncf) for b in (lo, hi)):
        raise ValueError(f"bounds must be a pair (lo, hi) of scalars or [{ncf}] vectors")
    lo, hi = (b.reshape(-1).expand(ncf).contiguous() for b in (lo, hi))
    if not bool((lo <= hi).all()):
        raise ValueError("bounds: lo must not exceed hi (and neither may be NaN)")
    s64 = st.double()
    if not bool(((s64 >= lo) & (s64 <= hi)).all()):
        raise ValueError("a start value lies outside its bounds (starts are not clamped)")
    return x, st, tg, z, mask, lo, hi


def fit_bias_table(beta1: float, beta2: float, iters: int) -> torch.Tensor:
    """[iters, 2] fp64: 1 - beta1**n and 1 - beta2**n for n = 1..iters, Python-float expressions evaluated on the host
    (as trainer.adam_bias_table: no pow on the device)."""
    return torch.tensor([(1 - beta1 ** float(n), 1 - beta2 ** float(n)) for n in range(1, iters + 1)],
                        dtype=torch.float64).reshape(iters, 2)


class _FitRun(_PositionRun):
    """The fit's run (R repeats per timestep): the optimiser state and a frozen train-structured workspace; a step ends
    with the frozen forward, ``cdm_fit_mse_grad``, the truncated backward and ``cdm_fit_grad_accum``.  ``cbuf`` is c32,
    the engine's input, written by ``cdm_fit_update``."""

    def __init__(self, pf: "ParamFit", M: int, Kc: int, npos: int, table: bool, R: int):
        super().__init__(pf, M, Kc, npos, table)
        self.R = R
        rows, ncf = self.cbuf.shape
        E = lambda *sh: torch.empty(*sh, device=pf.dev)
        I = lambda n: torch.zeros(n, dtype=torch.int32, device=pf.dev)
        D = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=pf.dev)
        self.deps, self.dc = E(*self.xt.shape), E(rows, ncf)
        self.c64, self.m, self.v, self.gacc = D(rows, ncf), D(rows, ncf), D(rows, ncf), D(rows, ncf)
        self.best_score, self.best_c = D(rows), E(rows, ncf)
        self.stalled, self.done = I(rows), I(1)

    def _workspace(self):
        return self.drv.eng.workspace(self.rows, True, frozen=True)

    def _score(self, s):
        pf, lb, nf = self.drv, lib(), self.drv.model.n_feat
        eps = pf.eng.forward(self.ws, pf.P, self.xt, self.t_cur, self.cbuf, self.sc_cur[:nf], self.sc_cur[nf:],
                             self.rows, s, frozen=True)
        lb.cdm_fit_mse_grad(_p(eps), _p(self.noise), self.M, self.Kc, self.HW, _p(self.cur_i), _p(pf.w), pf.T,
                            1.0 / self.R, _p(self.acc), self.Kc, 0, _p(self.deps), s)
        pf.eng.backward(self.ws, pf.P, self.deps, pf.G, s, dc=self.dc, stop_after="up0emb")
        lb.cdm_fit_grad_accum(_p(self.dc), self.rows, self.dc.shape[1], _p(self.gacc), s)

    def _cleared(self):
        return self.acc, self.gacc

    def load(self, x, c, *walk):
        super().load(x, c.to(self.drv.dev).reshape(self.rows, -1), *walk)     # row m Kc + k = start k of map m
        self.c64.copy_(self.cbuf)
        self.best_c.copy_(self.cbuf)
        self.best_score.fill_(float("inf"))
        for v in (self.m, self.v, self.gacc, self.acc, self.stalled, self.done, self.ctr):
            v.zero_()

    def run(self, iters, lr, b1, b2, eps, mask, lo, hi, bc, hist_s, hist_g):
        """iters + 1 passes over the positions, cdm_fit_update after each; the host reads nothing back."""
        lb, s = lib(), _s()
        for _ in range(iters + 1):
            self.positions()
            lb.cdm_fit_update(_p(self.done), iters, self.rows, self.cbuf.shape[1], _p(self.acc), _p(self.gacc), _p(mask),
                              _p(lo), _p(hi), lr, b1, b2, eps, _p(bc), _p(self.c64), _p(self.cbuf), _p(self.m),
                              _p(self.v), _p(self.best_score), _p(self.best_c), _p(hist_s), _p(hist_g),
                              _p(self.stalled), _p(self.ctr), s)


class ParamFit(_PositionDriver):
    """Fits the conditioning parameters of maps by gradient descent on the scan score (:class:`ParamScan` has the
    statistic; DESIGN §1 the definition).

    M maps, K starts per map c0[m, k]; the positions, the noise z_p[m] and the shortcut rows sc_p are the scan's, common
    to every start and to every iteration, so the objective is a deterministic function of c:
        eps_p[m,k] = model.eval()(x_p[m], t_p / T, c[m,k])     frozen-BatchNorm train-structured forward, batch M Kc
        score[m,k] = (1 / R) sum_p w[t_p] mean_pixels (eps_p[m,k] - z_p[m])^2                 fp64
        deps_p     = fp32(2 w[t_p] / (H W R)) (eps_p - z_p);   g[m,k,:] = sum_p dc_p[m,k,:]   dc_p fp32, the sum fp64
    and pass n = 1..iters evaluates score and g at the current c, records them, tracks the best, and takes one Adam
    step in fp64 clamped to the bounds (``cdm_fit_update``); pass iters + 1 evaluates the final c and only records.
    BatchNorm is frozen on the running statistics and GroupNorm is per sample, so rows do not interact.

    A step is ``cdm_scan_prologue``, the noise, ``cdm_scan_perturb``, the frozen forward, ``cdm_fit_mse_grad``, the
    engine backward stopped after the embeddings (``stop_after="up0emb"``: dc needs nothing below) and
    ``cdm_fit_grad_accum``; ``steps_per_graph`` steps are captured in one hipGraph and replayed, the rest and the
    update run eagerly; nothing is read back between iterations.  Starts go in chunks of Kc = max(1, max_rows // M):
    independent fits on the same positions, seed and shortcut rows (under h3 a row's arithmetic depends on its chunk
    through the per-tensor operand scale).  Cost: (iters + 1) P ceil(K / Kc) forward + backward pairs of M Kc rows.
    Shortcuts: one ``_draw_shortcut_row`` per position from the CPU RNG, once per call before any chunk runs — a fit
    and a scan after the same torch.manual_seed see the same objective.

    The fit runs on the engine's train pack (``repack(P, True)``, as a module call under autograd does): the pack token
    is renewed and the model's eval pack invalidated, so a Trainer, a pending autograd backward or an eval call sharing
    the engine afterwards repacks its own weights."""

    run_type = _FitRun

    def __init__(self, model, timesteps: int, steps_per_graph: int = 8, use_graph: bool = True, sched_tensors=None):
        super().__init__(model, timesteps, steps_per_graph, use_graph, sched_tensors)
        self._rehome(self.P)

    def _rehome(self, P):
        super()._rehome(P)
        # scratch parameter gradients of the truncated backward (written, never read)
        self.G = {n: torch.empty_like(P[n]) for n in self.model._param_names}

    def _repack(self):
        self.eng.repack(self.P, True, _s())
        self.eng.train_pack_token = object()
        self.model._invalidate_eval_pack()

    def fit(self, maps, start, iters=50, lr=0.02, free=None, bounds=(0.0, 1.0), betas=(0.9, 0.999), eps=1e-8,
            t_grid=None, n_steps=32, n_noise=1, weight="uniform", seed=4321, noise=None, max_rows=256) -> FitResult:
        m = self.model
        checked = check_fit(maps, start, self.T, m.n_cfeat, m.h, iters, lr, free, bounds, betas, eps, t_grid, n_steps,
                            n_noise, weight, noise, max_rows, m.in_channels)
        return self._fit(*checked, int(iters), float(lr), tuple(float(b) for b in betas), float(eps), int(n_noise),
                         weight, int(seed), int(max_rows))

    @torch.no_grad()
    def value_and_grad(self, maps, c, t_grid=None, n_steps=32, n_noise=1, weight="uniform", seed=4321, noise=None,
                       max_rows=256):
        """One evaluation of the objective at ``c`` ([ncf], [K, ncf] or [M, K, ncf]; no bounds apply): -> (score [M, K]
        fp64, g [M, K, ncf] fp64 = d score / d c), the quantities pass 1 of :meth:`fit` hands to the update.  Draws the
        shortcut rows as a fit does."""
        m = self.model
        big = float("inf")
        x, st, tg, z, _, _, _ = check_fit(maps, c, self.T, m.n_cfeat, m.h, 1, 1.0, None, (-big, big), (0.0, 0.0), 0.0,
                                          t_grid, n_steps, n_noise, weight, noise, max_rows, m.in_channels)
        M, K, ncf = st.shape
        score = torch.empty(M, K, dtype=torch.float64, device=self.dev)
        g = torch.empty(M, K, ncf, dtype=torch.float64, device=self.dev)
        R = int(n_noise)
        for sl, r in self._chunks(x, st, tg, z, R, weight, int(seed), int(max_rows), R):
            r.positions()
            score[:, sl] = r.acc
            g[:, sl] = r.gacc.view(M, -1, ncf)
        return score, g

    @torch.no_grad()
    def _fit(self, x, start, tg, z, mask, lo, hi, iters, lr, betas, eps, R, weight, seed, max_rows) -> FitResult:
        M, K, ncf = start.shape
        dev = self.dev
        mask, lo, hi = mask.to(dev), lo.to(dev), hi.to(dev)
        bc = fit_bias_table(betas[0], betas[1], iters).to(dev)
        D = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        score, hist_s, hist_g = D(M, K), D(iters + 1, M, K), D(iters + 1, M, K)
        params, last = torch.empty(M, K, ncf, device=dev), torch.empty(M, K, ncf, device=dev)
        stalled = torch.empty(M, K, dtype=torch.int32, device=dev)
        for sl, r in self._chunks(x, start, tg, z, R, weight, seed, max_rows, R):
            kc = r.Kc
            hs, hg = D(iters + 1, M * kc), D(iters + 1, M * kc)
            r.run(iters, lr, betas[0], betas[1], eps, mask, lo, hi, bc, hs, hg)
            score[:, sl] = r.best_score.view(M, kc)
            params[:, sl] = r.best_c.view(M, kc, ncf)
            last[:, sl] = r.cbuf.view(M, kc, ncf)
            stalled[:, sl] = r.stalled.view(M, kc)
            hist_s[:, :, sl] = hs.view(iters + 1, M, kc)
            hist_g[:, :, sl] = hg.view(iters + 1, M, kc)
        return FitResult(params, score, last, start.to(dev), hist_s, hist_g, stalled, tg, R, weight)


def param_fit(model, maps, start, timesteps, iters=50, lr=0.02, free=None, bounds=(0.0, 1.0), betas=(0.9, 0.999),
              eps=1e-8, t_grid=None, n_steps=32, n_noise=1, weight="uniform", seed=4321, noise=None, max_rows=256,
              steps_per_graph=8, ab_t=None, b_t=None) -> FitResult:
    """Descend the scan score of every map from every start: ``iters`` Adam steps in fp64 on the conditioning vector,
    clamped to ``bounds`` (:class:`ParamFit` has the definition, :class:`FitResult` the output).  ``maps`` [M, H, H] or
    [M, 1, H, H]; ``start`` [ncf], [K, ncf] (shared by all maps) or [M, K, ncf] — ``ScanResult.top(k)`` is the natural
    one; ``free``: the columns to fit (None = all; the others keep their bits); ``bounds``: (lo, hi), scalars or [ncf]
    vectors; ``t_grid``, ``n_steps``, ``n_noise``, ``weight``, ``seed``, ``noise``, ``max_rows``, ``ab_t`` / ``b_t`` as
    :func:`param_scan` takes them.  Costs (iters + 1) P ceil(K / Kc) forward + backward pairs of M Kc rows.

    The score is a ranking statistic, not a calibrated likelihood: the result is the minimiser of that
    statistic on one fixed draw of noise, a point estimate with no error bar.  Arguments are validated before anything
    touches the device or the CPU RNG (ValueError: :func:`check_fit`)."""
    sched = _sched_tensors(timesteps, ab_t, b_t, None)
    checked = check_fit(maps, start, timesteps, model.n_cfeat, model.h, iters, lr, free, bounds, betas, eps, t_grid,
                        n_steps, n_noise, weight, noise, max_rows, model.in_channels)
    pf = _cached(model, "_cdm_param_fit", (timesteps, int(steps_per_graph), sched),
                 lambda: ParamFit(model, timesteps, steps_per_graph, sched_tensors=sched))
    return pf._fit(*checked, int(iters), float(lr), tuple(float(b) for b in betas), float(eps), int(n_noise), weight,
                   int(seed), int(max_rows))


def calculate_elbo_and_bpd(*args, **kwargs):
    """Both reference signatures: (model, dataloader, timesteps, device, ab_t, b_t, a_t) from
    code/train_diffusion_paper.py:77 and (x, pred_noise, noise, t, b_t, a_t, ab_t, dims) from
    code/train_diffusion_elbo.py:74."""
    first = args[0] if args else kwargs.get("model", kwargs.get("x"))
    if torch.is_tensor(first):
        return calculate_elbo_and_bpd_batch(*args, **kwargs)
    return calculate_elbo_and_bpd_dataset(*args, **kwargs)
