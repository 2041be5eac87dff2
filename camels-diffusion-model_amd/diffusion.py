"""DDPM schedule, perturbation, denoising and the T-step (CFG) sampler on the HIP engine.

API mirrors the reference:
  schedule                      code/train_diffusion_condition.py:96-99
  perturb_input(x, t, noise)    :202-203   (non-standard (1 - ab) noise factor)
  denoise_add_noise(...)        :274-279
  sample_ddpm(n, size, device, params, guide_w)            :281-335  -> (x, intermediate)
  sample_ddpm_from_noise(noise_images, params, save_rate, guide_w)   :337-384
  functional sample_ddpm(model, ..., timesteps, b_t, a_t, ab_t)      code/sample_power_spectra.py:71-110
  unconditional reconstruction sampler                    code/train_diffusion.py:170-193

The sampler captures K denoise steps (prologue -> full ContextUnet eval forward -> fused
CFG-combine + denoise + snapshot) in one hipGraph and replays it; a device-side step counter makes
each captured step read its own timestep, coefficients, shortcut draw and noise stream, and the
reference's `intermediate.append(x.cpu())` snapshots are written on device into a preallocated
buffer (copied to host once at the end).

RNG modes (``z_source``):
  "device": z from on-device Philox; x_T / random params / per-forward shortcut draws consume the CPU
            RNG in exactly the order the reference's *GPU* run does (its z come from the CUDA generator).
  "host":   everything from the CPU RNG in the order of the reference's *CPU* run (x_T, then per step
            z then shortcut(s)); z is pre-drawn into a device table — bit-compatible with the oracle.

Strided sampling (DDIM, not in the reference): :class:`DDIMSampler` walks a subsequence of S of the T timesteps
(:func:`timestep_subsequence`) with the generalised update of :func:`ddim_tables` (eta = 0 deterministic, eta = 1 the
ancestral variance), on the same captured step graph; ``DDPM.sample_ddim`` / ``sample_ddim_from_noise`` and
``sample_ddpm(..., steps=S)`` are its entry points.  :class:`DPMSolverSampler` walks the same subsequence with the
second-order multistep update of :func:`dpmpp_tables` (DPM-Solver++ 2M: the previous step's data prediction is reused,
no extra network evaluation); ``DDPM.sample_dpm`` / ``sample_dpm_from_noise`` and ``sample_ddpm(..., steps=S,
solver="dpmpp")``.

Masked (inpainting) sampling (not in the reference): every sampler above takes ``known=`` / ``mask=`` and then
re-imposes the known pixels, noised to the level of the state (:func:`known_tables`), after every step with one more
kernel on the step graph (``cdm_mask_blend``; :class:`GraphSampler` has the definition); ``DDPM.inpaint`` is the
convenience entry point.

Position programs (not in the reference): the strided samplers take ``resample=`` / ``jump=`` (RePaint's resampling of a
masked run) and ``t_start=`` (a late start, SDEdit; ``DDPM.refine`` is its entry point) and then walk the positions of
:func:`resample_program` with per-position tables, a DDIM step keyed by the position and ``cdm_mask_blend_jump``
(:class:`_StridedSampler` has the definition).

Observation-guided sampling (not in the reference): ``DDPM.reconstruct`` draws maps consistent with a coarse, noisy,
partly missing observation (``degrade`` makes one): :class:`GuidedDDIMSampler` follows every DDIM step with a step down
the image gradient of the weighted misfit of the data prediction, one frozen forward and one full backward per position
on the step graph (``cdm_obs_residual_grad``, ``cdm_ddim_step_guided``).

Flow likelihood and DDIM encoding (not in the reference): ``DDPM.encode`` walks the sampler's timesteps upwards
(:class:`DDIMEncoder`, :func:`encode_tables`) from a map to its latent; ``DDPM.log_likelihood`` is the log-density of the
eta = 0 sampler by the change of variables along that walk (:class:`FlowLikelihood`: one frozen forward, one Rademacher
probe and one full backward per position on the step graph; ``cdm_flow_probe``, ``cdm_flow_step``, ``cdm_flow_finish``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from ._lib import lib

BETA1, BETA2 = 1e-4, 0.02


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _draw_shortcut_row(nf: int, sets: int = 1):
    """The random 1x1 shortcut conv(s) of one eval forward (diffusion_utilities.py:54), drawn from the CPU RNG as the
    reference constructs them -> [weights of every set, then biases]; ``sets`` = 2 with CFG: cond before uncond."""
    ws, bs = [], []
    for _ in range(sets):
        conv = nn.Conv2d(1, nf, kernel_size=1, stride=1, padding=0)
        ws.append(conv.weight.detach().reshape(nf)); bs.append(conv.bias.detach())
    return torch.cat(ws + bs)


def _capture_steps(warm_up, step, K: int):
    """The hipGraph of K calls of ``step(stream)``, captured on a side stream after one ``warm_up(stream)`` launch there
    (every kernel's code object resident before the capture)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm_up(s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(K):
            step(torch.cuda.current_stream().cuda_stream)
    return g


def _run_steps(graph, step, K: int, total: int):
    """``total`` steps on the current stream: replays of ``graph`` (K captured steps; None = no graph) while a whole one
    fits, then ``step(stream)`` eagerly for the rest."""
    done = 0
    if graph is not None:
        while done + K <= total:
            graph.replay()
            done += K
    s = _s()
    for _ in range(done, total):
        step(s)


def _rehomed(model, P):
    """The model's current parameter dict if any tensor of ``P`` changed address (a captured graph and a weight pack hold
    the old ones), else None."""
    new = model._engine_and_params()[1]
    return new if any(new[k].data_ptr() != v.data_ptr() for k, v in P.items()) else None


def sqrt_scalar_f32(v: torch.Tensor) -> torch.Tensor:
    """fp32 sqrt of every element as a 0-d tensor op computes it: IEEE correctly rounded, the same on every host
    (round(sqrt_fp64(x)) equals the correctly rounded fp32 sqrt: 53 >= 2 * 24 + 2 bits)."""
    return torch.from_numpy(np.sqrt(v.detach().cpu().double().numpy()).astype(np.float32))


class Schedule:
    """b_t, a_t, ab_t (T+1) computed with the reference's fp32 expressions on the host, plus the
    per-step coefficient tables the kernels read (same fp32 operations as the reference).

    The reference's denoise_add_noise (code/train_diffusion_condition.py:274-279) takes sqrt in two forms: of the whole
    vector, ``b_t.sqrt()[t]``, and of indexed 0-d scalars, ``a_t[t].sqrt()`` and ``(1 - ab_t[t]).sqrt()``.  torch's
    vectorised CPU sqrt is not correctly rounded and differs between hosts in a few entries (round 5: the MI355X box's
    host and the container that made the golden trajectories disagree in ``sqrt(b_t)``, ``sqrt(a_t)`` and
    ``sqrt(1 - ab_t)``, tools/traj_diag.py, profiles/r5_traj_diag.json), while the 0-d form is IEEE everywhere.  So the
    scalar forms are built with :func:`sqrt_scalar_f32` (host-independent, equal to the reference's values on any host)
    and the vector forms (``sqrt(b_t)`` here, ``sqrt(ab_t)`` of perturb_input, :202-203) with torch's vector sqrt on
    this host, as the reference evaluates them; ``sb`` replaces the latter with a given table (the trajectory parity
    tests pass the golden host's, tests/golden/schedule.npz)."""

    def __init__(self, timesteps: int, device="cuda", beta1: float = BETA1, beta2: float = BETA2, tensors=None,
                 sb: Optional[torch.Tensor] = None):
        """``tensors=(b_t, a_t, ab_t)`` uses a caller's schedule (the functional sampler of
        code/sample_power_spectra.py:71-110 takes them as arguments) instead of building the default one."""
        self.T = int(timesteps)
        if tensors is not None:
            b_t, a_t, ab_t = (torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1) for v in tensors)
            if not (b_t.numel() == a_t.numel() == ab_t.numel() == self.T + 1):
                raise ValueError(f"schedule tensors must have timesteps + 1 = {self.T + 1} entries")
        else:
            b_t = (beta2 - beta1) * torch.linspace(0, 1, self.T + 1) + beta1
            a_t = 1 - b_t
            ab_t = torch.cumsum(a_t.log(), dim=0).exp()
            ab_t[0] = 1
        dev = torch.device(device)
        self.b_t, self.a_t, self.ab_t = b_t.to(dev), a_t.to(dev), ab_t.to(dev)
        self.sab = ab_t.sqrt().to(dev)                       # perturb: ab_t.sqrt()[t] (vector form)
        self.omab = (1 - ab_t).to(dev)                       #          (1 - ab[t])
        # denoise: (1 - a_t[t]) / (1 - ab_t[t]).sqrt() and a_t[t].sqrt() (0-d forms), b_t.sqrt()[t] (vector form);
        # fp32 subtraction / division in numpy: IEEE like torch's
        oma = (1 - a_t).numpy()
        with np.errstate(divide="ignore", invalid="ignore"):   # entry 0 (1 - ab_t[0] = 0) is never used: t >= 1
            self.coef = torch.from_numpy((oma / sqrt_scalar_f32(1 - ab_t).numpy()).astype(np.float32)).to(dev)
        self.sa = sqrt_scalar_f32(a_t).to(dev)
        if sb is not None:
            sb = torch.as_tensor(sb).detach().to("cpu", torch.float32).reshape(-1)
            if sb.numel() != self.T + 1:
                raise ValueError(f"sb must have timesteps + 1 = {self.T + 1} entries")
            self.sb = sb.to(dev)
        else:
            self.sb = b_t.sqrt().to(dev)

    def tensors(self):
        return self.b_t, self.a_t, self.ab_t


def _as_i32(t, n, device):
    if isinstance(t, int) or (torch.is_tensor(t) and t.dim() == 0):
        return torch.full((n,), int(t), dtype=torch.int32, device=device)
    t = torch.as_tensor(t, device=device).reshape(-1).to(torch.int32)
    return t.expand(n).contiguous() if t.numel() == 1 else t.contiguous()


def perturb_input(x, t, noise, sched: Schedule):
    """sqrt(ab[t]) x + (1 - ab[t]) noise  (code/train_diffusion_condition.py:202-203); t int or [B]."""
    x = x.contiguous(); noise = noise.contiguous()
    B = x.shape[0]
    out = torch.empty_like(x)
    ti = _as_i32(t, B, x.device)
    lib().cdm_perturb(_p(x), _p(noise), _p(ti), None, 0, _p(sched.sab), _p(sched.omab), B, x[0].numel(), sched.T,
                      _p(out), None, _s())
    return out


def denoise_add_noise(x, t: int, pred_noise, z, sched: Schedule):
    """(x - eps (1-a)/sqrt(1-ab)) / sqrt(a) + sqrt(b) z   (code/train_diffusion_condition.py:274-279)."""
    x = x.contiguous(); pred_noise = pred_noise.contiguous()
    if z is None:
        z = torch.randn_like(x)
    if not torch.is_tensor(z):                      # the reference passes z = 0 at the last step
        z = torch.full_like(x, float(z))
    z = z.contiguous()
    out = torch.empty_like(x)
    cur = torch.full((1,), int(t), dtype=torch.int32, device=x.device)
    T = max(int(t), sched.T)
    # z_table with stride 0: z[e] for every step; force i > 1 semantics by the table itself
    lib().cdm_denoise(_p(x), _p(out), None, x.numel(), _p(pred_noise), 0, 0.0, _p(cur), _p(sched.coef),
                      _p(sched.sa), _p(sched.sb), _p(z), 0, 0, None, None, None, T, _s())
    if int(t) <= 1 and z.abs().max().item() != 0:  # kernel treats i == 1 as z = 0 (reference passes 0 there)
        out = out + sched.b_t.sqrt()[int(t)] * z
    return out


def snapshot_slots(T: int, save_rate: int = 20):
    """slot index per step i (reference: i % save_rate == 0 or i == T or i < 8), in append order."""
    slots = np.full(T + 1, -1, dtype=np.int32)
    k = 0
    for i in range(T, 0, -1):
        if i % save_rate == 0 or i == T or i < 8:
            slots[i] = k
            k += 1
    return slots, k


def timestep_subsequence(T: int, S: Optional[int] = None, spacing="uniform"):
    """The timesteps tau_1 < ... < tau_S = T a strided sampler visits (in reverse), as a list of ints.

    ``spacing``: ``"uniform"``: tau_k = round(k T / S) (halves round up); ``"quadratic"``: tau_k = max(ceil(T (k/S)^2), k)
    (denser near t = 0); or an explicit increasing sequence of ints (``S`` is then None or its length).  Pure host
    function.  Raises ValueError unless 1 <= tau_1, the sequence is strictly increasing and tau_S == T; nothing is
    repaired."""
    T = int(T)
    if T < 1:
        raise ValueError("T must be >= 1")
    if isinstance(spacing, str):
        if S is None or int(S) != S or int(S) < 1:
            raise ValueError(f"steps must be a positive integer, got {S!r}")
        S = int(S)
        if S > T:
            raise ValueError(f"steps = {S} exceeds the {T} timesteps of the schedule")
        if spacing == "uniform":
            tau = [(2 * k * T + S) // (2 * S) for k in range(1, S + 1)]          # exact integer round-half-up
        elif spacing == "quadratic":
            tau = [max(-((-T * k * k) // (S * S)), k) for k in range(1, S + 1)]    # exact integer ceil
        else:
            raise ValueError(f"spacing must be 'uniform', 'quadratic' or a list of timesteps, got {spacing!r}")
    else:
        raw = [v.item() if hasattr(v, "item") else v for v in spacing]
        if any(isinstance(v, bool) or int(v) != v for v in raw):
            raise ValueError("an explicit timestep list must hold integers")
        tau = [int(v) for v in raw]
        if S is not None and int(S) != len(tau):
            raise ValueError(f"steps = {S} but the explicit timestep list has {len(tau)} entries")
    if not tau:
        raise ValueError("the timestep list is empty")
    if tau[0] < 1:
        raise ValueError(f"the first timestep must be >= 1, got {tau[0]}")
    if any(b <= a for a, b in zip(tau, tau[1:])):
        raise ValueError("the timesteps must be strictly increasing")
    if tau[-1] != T:
        raise ValueError(f"the last timestep must be T = {T}, got {tau[-1]}")
    return tau


def ddim_tables(ab_t, taus, eta: float = 0.0):
    """Coefficient tables (cx, ce, sigma) of the strided update, fp32 numpy arrays of S + 1 entries indexed by the
    position k = 1..S (entry 0 is the unused identity 1, 0, 0).

    With tau_0 = 0 (ab_0 = 1), a step from i = tau_k to j = tau_{k-1} is

        sigma = eta sqrt((1 - ab_j) / (1 - ab_i)) sqrt(1 - ab_i / ab_j)
        cx    = sqrt(ab_j / ab_i)
        ce    = sqrt(1 - ab_j - sigma^2) - sqrt(ab_j (1 - ab_i) / ab_i)
        x_j   = cx x_i + ce eps + sigma z                 (sigma = 0, no z, when j = 0)

    This is DDIM (Song et al. 2021, eq. 12) in the convention of the reference's *sampler*, whose denoise_add_noise
    (code/train_diffusion_condition.py:274-279) treats the network output as the noise of x = sqrt(ab) x0 +
    sqrt(1 - ab) eps: over the full sequence 1..T with eta = 1 the tables are that function's 1 / sqrt(a),
    -(1 - a) / (sqrt(1 - ab) sqrt(a)) and the posterior variance b (1 - ab_{t-1}) / (1 - ab_t).  It does not follow
    the (1 - ab) noise factor of perturb_input (:202-203), which the reference's own sampler ignores too.

    ``ab_t`` is the fp32 table of the Schedule (T + 1 entries); the arithmetic is fp64 numpy, rounded once to fp32, so
    the tables do not depend on the host's vectorised fp32 sqrt (the concern of :func:`sqrt_scalar_f32`).  Pure host
    function."""
    if torch.is_tensor(ab_t):
        ab_t = ab_t.detach().cpu().numpy()
    ab = np.asarray(ab_t, dtype=np.float32).astype(np.float64).reshape(-1)
    eta = float(eta)
    if not (eta >= 0.0) or not np.isfinite(eta):
        raise ValueError(f"eta must be finite and >= 0, got {eta}")
    tau = timestep_subsequence(ab.size - 1, None, taus)
    S = len(tau)
    i = np.array(tau, dtype=np.int64)
    j = np.array([0] + tau[:-1], dtype=np.int64)
    ab_i, ab_j = ab[i], ab[j]
    ab_j[0] = 1.0                                             # tau_0 = 0: ab_0 = 1 by definition
    with np.errstate(divide="ignore", invalid="ignore"):     # a degenerate schedule is reported below
        sigma = eta * np.sqrt((1 - ab_j) / (1 - ab_i)) * np.sqrt(1 - ab_i / ab_j)
        sigma[0] = 0.0
        rad = 1 - ab_j - sigma * sigma
        if (rad < 0).any():
            raise ValueError(f"eta = {eta} makes sigma^2 exceed 1 - ab_j at position {int(np.argmax(rad < 0)) + 1}")
        cx = np.sqrt(ab_j / ab_i)
        ce = np.sqrt(rad) - np.sqrt(ab_j * (1 - ab_i) / ab_i)
    out = []
    for v, v0 in ((cx, 1.0), (ce, 0.0), (sigma, 0.0)):
        if not np.isfinite(v).all():
            raise ValueError("the schedule gives non-finite DDIM coefficients (ab_t must lie in (0, 1) for t >= 1)")
        out.append(np.concatenate([[v0], v]).astype(np.float32))
    assert all(o.size == S + 1 for o in out)
    return tuple(out)


def dpmpp_tables(ab_t, taus, order: int = 2, dtype=np.float32):
    """Coefficient tables (sq, ra, c0, c1, cx, cd) of the multistep update DPM-Solver++(2M) (Lu et al. 2022, algorithm
    2), numpy arrays of S + 1 entries indexed by the position k = 1..S (entry 0 is the unused 0, 1, 1, 0, 1, 0).

    With tau_0 = 0 (ab_0 = 1), alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma), a step from
    i = tau_k to j = tau_{k-1} with h_k = lambda_j - lambda_i (h_1 = +inf) is

        sq = sigma_i,  ra = 1 / alpha_i                  d   = (x_i - sq eps) ra            (data prediction)
        c0 = 1 + 1 / (2 r),  c1 = -1 / (2 r)             D   = c0 d + c1 d_prev             (r = h_{k+1} / h_k)
        cx = sigma_j / sigma_i                           x_j = cx x_i + cd D ;  d_prev <- d
        cd = alpha_j - sigma_j alpha_i / sigma_i         (= alpha_j (1 - e^{-h_k});  cx[1] = 0, cd[1] = 1)

    The first position (k = S, no d_prev yet) and the last (k = 1, the step to t = 0) are first order, c0 = 1 and
    c1 = 0, and so is every position with ``order=1``; c1 == 0 means D = d and d_prev is not read.  S <= 2 is therefore
    first order throughout.  The first-order update is DDIM at eta = 0: cx + cd ra and -cd ra sq are ddim_tables' cx
    and ce.  The noise convention is the sampler's, sqrt(1 - ab), as :func:`ddim_tables` documents.

    ``ab_t`` is the fp32 table of the Schedule (T + 1 entries); the arithmetic is fp64 numpy, rounded once to ``dtype``
    (np.float32 for the kernel; np.float64 returns the unrounded values).  Pure host function.  Raises ValueError for an
    order other than 1 or 2 and for a schedule that gives non-finite coefficients or a non-increasing lambda."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    if torch.is_tensor(ab_t):
        ab_t = ab_t.detach().cpu().numpy()
    ab = np.asarray(ab_t, dtype=np.float32).astype(np.float64).reshape(-1)
    tau = timestep_subsequence(ab.size - 1, None, taus)
    S = len(tau)
    i = np.array(tau, dtype=np.int64)
    j = np.array([0] + tau[:-1], dtype=np.int64)
    ab_i, ab_j = ab[i], ab[j]
    ab_j[0] = 1.0                                             # tau_0 = 0: ab_0 = 1 by definition
    bad = ValueError("the schedule gives non-finite DPM-Solver++ coefficients (ab_t must lie in (0, 1) for t >= 1 and "
                     "decrease along the timesteps)")
    with np.errstate(divide="ignore", invalid="ignore"):     # a degenerate schedule is reported below
        al_i, al_j = np.sqrt(ab_i), np.sqrt(ab_j)
        sg_i, sg_j = np.sqrt(1 - ab_i), np.sqrt(1 - ab_j)
        sq, ra = sg_i, 1 / al_i
        cx = sg_j / sg_i
        cd = al_j - sg_j * al_i / sg_i
        h = np.log(al_j / sg_j) - np.log(al_i / sg_i)        # h[0] = h_1 = +inf (sigma_j = 0)
        c0, c1 = np.ones(S), np.zeros(S)
        if order == 2 and S > 2:
            r = h[2:] / h[1:-1]                               # positions k = 2..S-1: h_{k+1} / h_k
            c0[1:-1], c1[1:-1] = 1 + 1 / (2 * r), -1 / (2 * r)
    if not (h[1:] > 0).all() or not h[0] > 0:
        raise bad
    out = []
    for v, v0 in ((sq, 0.0), (ra, 1.0), (c0, 1.0), (c1, 0.0), (cx, 1.0), (cd, 0.0)):
        if not np.isfinite(v).all():
            raise bad
        out.append(np.concatenate([[v0], v]).astype(dtype))
    assert all(o.size == S + 1 for o in out)
    return tuple(out)


def known_tables(ab_t):
    """(sab, somab) of masked sampling: sqrt(ab_t) and sqrt(1 - ab_t), fp32 numpy arrays of T + 1 entries indexed by the
    timestep; sab[0] = 1 and somab[0] = 0 exactly (ab_0 = 1 by definition).

    A known pixel is carried at the noise level of the state it is blended into, kn_j = sab[j] known + somab[j] xi: the
    noise convention of the sampler (:func:`ddim_tables`), not perturb_input's (1 - ab).  ``ab_t`` is the fp32 table of
    the Schedule; the arithmetic is fp64 numpy, rounded once to fp32, as in ddim_tables.  Pure host function.  Raises
    ValueError on a non-finite entry (ab_t outside [0, 1])."""
    if torch.is_tensor(ab_t):
        ab_t = ab_t.detach().cpu().numpy()
    ab = np.asarray(ab_t, dtype=np.float32).astype(np.float64).reshape(-1)
    if ab.size < 2:
        raise ValueError("ab_t must have T + 1 >= 2 entries")
    ab[0] = 1.0                                               # ab_0 = 1 by definition
    with np.errstate(invalid="ignore"):                      # reported below
        sab, somab = np.sqrt(ab), np.sqrt(1 - ab)
    if not (np.isfinite(sab).all() and np.isfinite(somab).all()):
        raise ValueError("the schedule gives non-finite known-region tables (ab_t must lie in [0, 1])")
    return sab.astype(np.float32), somab.astype(np.float32)


def guided_tables(ab_t, taus):
    """(sq, ra) of observation-guided sampling: sqrt(1 - ab_i) and 1 / sqrt(ab_i) at i = tau_p, fp32 numpy arrays of
    S + 1 entries indexed by the position p = 1..S (entry 0 is the unused 0, 1), so that the data prediction of a state is
    x0h = (x - sq[p] eps) ra[p] (:func:`dpmpp_tables`' first two tables).  ``ab_t`` is the fp32 table of the Schedule;
    the arithmetic is fp64 numpy, rounded once to fp32.  Pure host function.  Raises ValueError for an invalid ``taus``
    (:func:`timestep_subsequence`) and for a schedule that gives a non-finite entry (ab_t must lie in (0, 1])."""
    ab = _ab64(ab_t)
    tau = timestep_subsequence(ab.size - 1, None, taus)
    ab_i = ab[np.array(tau, dtype=np.int64)]
    with np.errstate(divide="ignore", invalid="ignore"):     # reported below
        sq, ra = np.sqrt(1 - ab_i), 1 / np.sqrt(ab_i)
    if not (np.isfinite(sq).all() and np.isfinite(ra).all()):
        raise ValueError("the schedule gives non-finite guidance tables (ab_t must lie in (0, 1] for t >= 1)")
    return (np.concatenate([[0.0], sq]).astype(np.float32), np.concatenate([[1.0], ra]).astype(np.float32))


def encode_tables(ab_t, taus):
    """Tables (from_t int32, ix fp32, ie fp32, g fp64) of the ascending (encoding) walk over ``taus``, S + 1 entries
    indexed by the position p = S..1 in run order: position p performs the step k = S + 1 - p, from tau_{k-1} to tau_k,
    with the network seeing the state at from_t[p] = tau_k (the usual DDIM-inversion convention: the walk visits the
    sampler's timesteps and never t = 0).  With (cx_k, ce_k) the eta = 0 coefficients of :func:`ddim_tables` in fp64,

        x <- ix x + ie eps        ix = 1 / cx_k,   ie = -ce_k / cx_k,   g = ie / ix = -ce_k

    the inverse of the sampler's step at a fixed eps; the step's Jacobian is ix (I + g d eps / d x).  Entry 0 is the
    identity (0, 1, 0, 0).  ``ab_t`` is the fp32 table of the Schedule; the arithmetic is fp64 numpy, ix and ie rounded
    once to fp32, g kept in fp64 (the log-determinant is accumulated in fp64).  Pure host function.  Raises ValueError
    for an invalid ``taus`` (:func:`timestep_subsequence`) and for a schedule that gives a non-finite entry."""
    ab = _ab64(ab_t)
    tau = timestep_subsequence(ab.size - 1, None, taus)
    i = np.array(tau, dtype=np.int64)
    j = np.array([0] + tau[:-1], dtype=np.int64)
    ab_i, ab_j = ab[i], ab[j]
    ab_j[0] = 1.0                                             # tau_0 = 0: ab_0 = 1 by definition
    with np.errstate(divide="ignore", invalid="ignore"):     # a degenerate schedule is reported below
        cx = np.sqrt(ab_j / ab_i)
        ce = np.sqrt(1 - ab_j) - np.sqrt(ab_j * (1 - ab_i) / ab_i)
        ix, ie, g = 1 / cx, -ce / cx, -ce
    out = []
    for v, v0, dt in ((ix, 1.0, np.float32), (ie, 0.0, np.float32), (g, 0.0, np.float64)):
        if not np.isfinite(v).all() or not np.isfinite(v.astype(dt)).all():
            raise ValueError("the schedule gives non-finite encoding coefficients (ab_t must lie in (0, 1) for t >= 1)")
        out.append(np.concatenate([[v0], v[::-1]]).astype(dt))           # step k at the position S + 1 - k
    from_t = np.array([0] + tau[::-1], dtype=np.int32)
    return (from_t, *out)


FLOW_FORMS = ("trace", "logdet")
_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def flow_run_key(seed: int, r: int) -> int:
    """The 64-bit run key of probe run ``r`` under ``seed``: splitmix64(splitmix64(seed) + r mod 2^64) (Steele et al.
    2014, the finaliser of java.util.SplittableRandom).  splitmix64 is a bijection, so two pairs (seed, r) share a key
    only if splitmix64(seed) - splitmix64(seed') = r' - r: neighbouring seeds do not share probes, and results pooled
    over seeds are as independent as results over r.  Pure host function."""
    return _splitmix64((_splitmix64(int(seed) & _M64) + int(r)) & _M64)


def check_flow(maps, params, n_cfeat: int, H: int, in_channels: int = 1, guide_w: float = 0.0, form: str = "logdet",
               n_probe: int = 1, max_rows: int = 32):
    """Validate the inputs of ``DDPM.log_likelihood`` -> (maps [n,1,H,H], params [n,n_cfeat] or None) as given (any
    device); ``maps`` may come without the channel axis.  Pure host function.  ValueError, before anything is allocated
    or drawn: ``guide_w`` != 0 (the density is that of the unguided sampler: the CFG combination of two networks has
    its own Jacobian, which is not built); a model with in_channels > 1; ``form`` not "logdet" or "trace"; ``n_probe``
    or ``max_rows`` not an integer >= 1; maps not [n,1,H,H] / [n,H,H] with n >= 1, not floating point or non-finite;
    params not [n, n_cfeat], not floating point or non-finite."""
    if isinstance(guide_w, bool) or not float(guide_w) == 0.0:
        raise ValueError(f"log_likelihood is the density of the unguided sampler: guide_w must be 0, got {guide_w!r}")
    if in_channels != 1:
        raise ValueError(f"log_likelihood is single-channel, like the samplers: the model has in_channels = {in_channels}")
    if form not in FLOW_FORMS:
        raise ValueError(f"form must be one of {FLOW_FORMS}, got {form!r}")
    _posint("n_probe", n_probe)
    _posint("max_rows", max_rows)
    x = torch.as_tensor(maps)
    if x.dim() == 3:
        x = x[:, None]
    if x.dim() != 4 or tuple(x.shape[1:]) != (1, H, H) or x.shape[0] < 1:
        raise ValueError(f"maps must have shape [n, 1, {H}, {H}] or [n, {H}, {H}], got {tuple(torch.as_tensor(maps).shape)}")
    if not x.is_floating_point() or not bool(torch.isfinite(x).all()):
        raise ValueError("maps must be a finite floating-point array")
    if params is not None:
        params = torch.as_tensor(params)
        if tuple(params.shape) != (x.shape[0], n_cfeat):
            raise ValueError(f"params must have shape {(x.shape[0], n_cfeat)}, got {tuple(params.shape)}")
        if not params.is_floating_point() or not bool(torch.isfinite(params).all()):
            raise ValueError("params must be a finite floating-point array")
    return x, params


class FlowResult(NamedTuple):
    """What ``DDPM.log_likelihood`` returns: host tensors, fp64 unless noted.  ``logp`` is the log-density, per map, of
    the eta = 0 sampler's model at guide_w = 0, in the sampler's noise convention, discretised at S positions, with a
    stochastic trace estimate.  It is not a bound, and the reference does not compute it."""
    logp: torch.Tensor          # [n]: the mean over the probes
    logp_probe: torch.Tensor    # [R, n]: one value per probe run
    stderr: torch.Tensor        # [n]: the standard error of that mean over the probes; NaN for R = 1
    bpd: torch.Tensor           # [n]: -logp / (D ln 2) on the model's own data scale, no dequantisation offset
    latent: torch.Tensor        # [n, 1, H, H] fp32: the encoded x_T (the same for every probe)
    prior: torch.Tensor         # [n]: log N(x_T; 0, I)
    logdet: torch.Tensor        # [n]: (D / 2) log ab_T + sum_k ld_k, the mean over the probes
    trace_hist: torch.Tensor    # [R, S, n]: q_k = v^T J_k v in step order k = 1..S
    invalid: torch.Tensor       # [n] bool: a non-finite ld_k in any probe run (logp is then NaN)
    taus: list                  # the timesteps tau_1 < ... < tau_S = T of the walk


class Program(NamedTuple):
    """A position program (:func:`resample_program`): arrays of P + 1 entries indexed by the position p = P..1 in the
    order it runs, entry 0 unused."""
    from_t: np.ndarray      # int32: the timestep i the network sees
    land_t: np.ndarray      # int32: the timestep j the update lands on
    up_t: np.ndarray        # int32: the timestep u the state is re-noised to after the blend; == land_t: no jump
    fa: np.ndarray          # fp32: sqrt(ab_u / ab_j); 1 exactly where there is no jump
    fb: np.ndarray          # fp32: sqrt(1 - ab_u / ab_j); 0 exactly where there is no jump

    @property
    def P(self) -> int:
        return self.from_t.size - 1


def _ab64(ab_t):
    if torch.is_tensor(ab_t):
        ab_t = ab_t.detach().cpu().numpy()
    return np.asarray(ab_t, dtype=np.float32).astype(np.float64).reshape(-1)


def _posint(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(v)


def resample_program(ab_t, taus, jump: int = 1, resamples: int = 1, t_start: Optional[int] = None) -> Program:
    """The walk over the timesteps ``taus`` (ascending, :func:`timestep_subsequence`; tau_0 = 0) of a run with RePaint's
    resampling jumps (Lugmayr et al. 2022, get_schedule_jump) and / or a late start (SDEdit) -> :class:`Program`.

    Late start: only the taus <= ``t_start`` are kept (S' of them; None keeps all) and the run starts at tau_S'.
    Resampling, ``resamples`` = R and ``jump`` = J counted in positions: the state indices k that are multiples of J with
    J <= k <= S' - J are jump points, each good for R - 1 jumps.  From k = S', while k > 0: emit a position from
    i = tau_k landing on j = tau_{k-1}; k -= 1; if k is a jump point with jumps left, use one: the position just emitted
    is marked with the target u = tau_{k+J} (after its blend the state is re-noised from j to u,
    x_u = fa x_j + fb zeta with fa = sqrt(ab_u / ab_j), fb = sqrt(1 - ab_u / ab_j)) and k += J.  A used jump is never
    restored.  P = S' + (R - 1) J (S' // J - 1) positions; the first emitted is p = P, the last p = 1.

    ``ab_t`` is the fp32 table of the Schedule; the arithmetic is fp64 numpy, rounded once to fp32, as in
    :func:`ddim_tables`.  Pure host function.  ValueError: ``taus`` not a valid subsequence of 1..T, ``jump`` or
    ``resamples`` not an integer >= 1, ``t_start`` outside 1..T or below tau_1, R > 1 with no jump point (S' < 2 J)."""
    ab = _ab64(ab_t)
    T = ab.size - 1
    tau = timestep_subsequence(T, None, taus)
    J, R = _posint("jump", jump), _posint("resamples", resamples)
    if t_start is not None:
        if isinstance(t_start, bool) or int(t_start) != t_start or not 1 <= int(t_start) <= T:
            raise ValueError(f"t_start must be an integer in 1..T = {T}, got {t_start!r}")
        tau = [t for t in tau if t <= int(t_start)]
        if not tau:
            raise ValueError(f"t_start = {t_start} lies below the first timestep of the run")
    S = len(tau)
    if R > 1 and S < 2 * J:
        raise ValueError(f"resamples = {R} needs a jump point: {S} positions are fewer than 2 * jump = {2 * J}")
    tau = [0] + tau
    left = {k: R - 1 for k in range(J, S - J + 1, J)}
    frm, land, up = [0], [0], [0]
    k = S
    while k > 0:
        frm.append(tau[k]); land.append(tau[k - 1]); up.append(tau[k - 1])
        k -= 1
        if left.get(k, 0) > 0:
            left[k] -= 1
            up[-1] = tau[k + J]
            k += J
    P = len(frm) - 1
    assert P == S + (R - 1) * J * (S // J - 1 if S >= 2 * J else 0)
    frm, land, up = (np.array(v[:1] + v[:0:-1], dtype=np.int64) for v in (frm, land, up))   # emitted first = position P
    ab[0] = 1.0                                               # tau_0 = 0: ab_0 = 1 by definition
    with np.errstate(divide="ignore", invalid="ignore"):     # reported below
        ratio = ab[up] / ab[land]
        fa, fb = np.sqrt(ratio), np.sqrt(1 - ratio)
    stay = up == land
    fa[stay], fb[stay] = 1.0, 0.0
    if not (np.isfinite(fa).all() and np.isfinite(fb).all()):
        raise ValueError("the schedule gives non-finite jump tables (ab_t must lie in (0, 1] and decrease)")
    return Program(frm.astype(np.int32), land.astype(np.int32), up.astype(np.int32), fa.astype(np.float32),
                   fb.astype(np.float32))


def _pairs(ab_t, from_t, land_t):
    """(i, j, ab_i, ab_j) of the positions 1..P of a program's (from_t, land_t) tables, validated."""
    ab = _ab64(ab_t)
    i, j = (np.asarray(v).astype(np.int64).reshape(-1)[1:] for v in (from_t, land_t))
    if i.size < 1 or i.size != j.size:
        raise ValueError("from_t and land_t must have the same P + 1 >= 2 entries")
    if (j < 0).any() or (i <= j).any() or (i >= ab.size).any():
        raise ValueError(f"every position must descend, 0 <= land_t < from_t <= T = {ab.size - 1}")
    ab_i, ab_j = ab[i], ab[j]
    ab_j[j == 0] = 1.0                                        # tau_0 = 0: ab_0 = 1 by definition
    return i, j, ab_i, ab_j


def ddim_tables_from_pairs(ab_t, from_t, land_t, eta: float = 0.0):
    """:func:`ddim_tables` for the positions of a :class:`Program`: (cx, ce, sigma) of P + 1 entries, the step of
    position p going from from_t[p] to land_t[p] (entry 0 of the two is ignored).  The same expressions on the same
    numbers: for the plain program of ``taus`` (no jump, no late start) the result is ddim_tables' bit for bit."""
    eta = float(eta)
    if not (eta >= 0.0) or not np.isfinite(eta):
        raise ValueError(f"eta must be finite and >= 0, got {eta}")
    i, j, ab_i, ab_j = _pairs(ab_t, from_t, land_t)
    with np.errstate(divide="ignore", invalid="ignore"):     # a degenerate schedule is reported below
        sigma = eta * np.sqrt((1 - ab_j) / (1 - ab_i)) * np.sqrt(1 - ab_i / ab_j)
        sigma[j == 0] = 0.0
        rad = 1 - ab_j - sigma * sigma
        if (rad < 0).any():
            raise ValueError(f"eta = {eta} makes sigma^2 exceed 1 - ab_j at position {int(np.argmax(rad < 0)) + 1}")
        cx = np.sqrt(ab_j / ab_i)
        ce = np.sqrt(rad) - np.sqrt(ab_j * (1 - ab_i) / ab_i)
    out = []
    for v, v0 in ((cx, 1.0), (ce, 0.0), (sigma, 0.0)):
        if not np.isfinite(v).all():
            raise ValueError("the schedule gives non-finite DDIM coefficients (ab_t must lie in (0, 1) for t >= 1)")
        out.append(np.concatenate([[v0], v]).astype(np.float32))
    return tuple(out)


def dpmpp_tables_from_pairs(ab_t, from_t, land_t, up_t=None, order: int = 2, dtype=np.float32):
    """:func:`dpmpp_tables` for the positions of a :class:`Program`: (sq, ra, c0, c1, cx, cd) of P + 1 entries.

    Position p is second order (c1 != 0) only if the position before it exists (p < P), that position had no jump after
    it (up_t[p + 1] == land_t[p + 1]; ``up_t`` None: no jumps) and p does not land on 0; then r = h_{p+1} / h_p with that
    previous position's own h.  After a jump the history is dropped, c1 = 0 as at the first position: the kept data
    prediction belongs to a state that was re-noised since.  The same expressions on the same numbers as dpmpp_tables:
    bit-equal to it for the plain program of ``taus``."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    i, j, ab_i, ab_j = _pairs(ab_t, from_t, land_t)
    P = i.size
    land = np.asarray(land_t).astype(np.int64).reshape(-1)[1:]
    up = land if up_t is None else np.asarray(up_t).astype(np.int64).reshape(-1)[1:]
    if up.size != P:
        raise ValueError("up_t must have the P + 1 entries of from_t")
    bad = ValueError("the schedule gives non-finite DPM-Solver++ coefficients (ab_t must lie in (0, 1) for t >= 1 and "
                     "decrease along the timesteps)")
    with np.errstate(divide="ignore", invalid="ignore"):     # a degenerate schedule is reported below
        al_i, al_j = np.sqrt(ab_i), np.sqrt(ab_j)
        sg_i, sg_j = np.sqrt(1 - ab_i), np.sqrt(1 - ab_j)
        sq, ra = sg_i, 1 / al_i
        cx = sg_j / sg_i
        cd = al_j - sg_j * al_i / sg_i
        h = np.log(al_j / sg_j) - np.log(al_i / sg_i)        # +inf where the position lands on 0 (sigma_j = 0)
        c0, c1 = np.ones(P), np.zeros(P)
        if order == 2 and P > 1:
            second = np.zeros(P, dtype=bool)
            second[:-1] = (up[1:] == land[1:]) & (j[:-1] != 0)
            q = np.nonzero(second)[0]
            r = h[q + 1] / h[q]
            c0[q], c1[q] = 1 + 1 / (2 * r), -1 / (2 * r)
    if not (h > 0).all():
        raise bad
    out = []
    for v, v0 in ((sq, 0.0), (ra, 1.0), (c0, 1.0), (c1, 0.0), (cx, 1.0), (cd, 0.0)):
        if not np.isfinite(v).all():
            raise bad
        out.append(np.concatenate([[v0], v]).astype(dtype))
    return tuple(out)


def _program(ab_t, taus, resample, jump, t_start, inpaint):
    """The program of a strided sampler's (resample, jump, t_start), or None when all three are at their defaults: the
    plain walk, which keeps the kernels, buffers and RNG walk it had before programs existed.  ValueError: what
    :func:`resample_program` raises, and resample > 1 on a sampler without a mask (there is nothing to harmonise)."""
    if (resample, jump, t_start) == (1, 1, None) and not any(isinstance(v, bool) for v in (resample, jump)):
        return None
    prog = resample_program(ab_t, taus, jump, resample, t_start)
    if resample > 1 and inpaint is None:
        raise ValueError("resample > 1 re-noises towards a known region: it needs masked sampling (known= and mask=)")
    return prog


KNOWN_NOISE_MODES = ("fixed", "fresh")


def check_inpaint(known, mask, n: int, H: int, known_noise: str = "fixed", in_channels: int = 1):
    """Validate the inputs of masked sampling -> (known [n,1,H,H], mask [n or 1,1,H,H]) as given (any device), or
    (None, None) when neither is given.  ValueError: an unknown ``known_noise``; one of known / mask without the other;
    a model with in_channels > 1; a shape other than those; a mask value non-finite or outside [0, 1]; ``known``
    non-finite where mask > 0 (where the mask is 0 it is never used and may hold anything)."""
    if known_noise not in KNOWN_NOISE_MODES:
        raise ValueError(f"known_noise must be one of {KNOWN_NOISE_MODES}, got {known_noise!r}")
    if known is None and mask is None:
        return None, None
    if known is None or mask is None:
        raise ValueError("masked sampling needs both known= and mask=")
    if in_channels != 1:
        raise ValueError("masked sampling is single-channel, like the samplers: the model has in_channels = "
                         f"{in_channels}")
    known, mask = torch.as_tensor(known), torch.as_tensor(mask)
    if tuple(known.shape) != (n, 1, H, H):
        raise ValueError(f"known must have shape {(n, 1, H, H)}, got {tuple(known.shape)}")
    if tuple(mask.shape) not in ((n, 1, H, H), (1, 1, H, H)):
        raise ValueError(f"mask must have shape {(n, 1, H, H)} or {(1, 1, H, H)}, got {tuple(mask.shape)}")
    if not (known.is_floating_point() and mask.is_floating_point()):
        raise ValueError("known and mask must be floating-point arrays")
    if not bool(((mask >= 0) & (mask <= 1)).all()):          # NaN fails both comparisons
        raise ValueError("mask values must be finite and lie in [0, 1]")
    if not bool(torch.isfinite(known)[(mask > 0).expand_as(known)].all()):
        raise ValueError("known holds a non-finite value where mask > 0")
    return known, mask


OBS_FACTORS = (1, 2, 4, 8)


def check_observation(obs, weight, n: int, H: int, factor: int = 4, zeta: float = 1.0, in_channels: int = 1):
    """Validate the inputs of observation-guided sampling -> (obs [n,1,h,h], weight [n or 1,1,h,h]) with h = H / factor,
    as given (any device); ``weight`` None is the plane of ones [1,1,h,h].  ``obs`` and ``weight`` may come without the
    channel axis.  ValueError, before anything is allocated: a model with in_channels > 1; ``factor`` not in
    {1, 2, 4, 8} or not dividing H; ``zeta`` negative or not finite; a shape other than those; a non-floating array; a
    weight negative or non-finite; ``obs`` non-finite where the weight is > 0 (where it is 0 the cell is not observed and
    may hold anything)."""
    if in_channels != 1:
        raise ValueError("observation-guided sampling is single-channel, like the samplers: the model has in_channels "
                         f"= {in_channels}")
    if isinstance(factor, bool) or factor not in OBS_FACTORS:
        raise ValueError(f"factor must be one of {OBS_FACTORS}, got {factor!r}")
    if H % factor != 0:
        raise ValueError(f"factor = {factor} does not divide the map size {H}")
    if isinstance(zeta, bool) or not np.isfinite(zeta) or not zeta >= 0:
        raise ValueError(f"zeta must be finite and >= 0, got {zeta!r}")
    if obs is None:
        raise ValueError("observation-guided sampling needs obs=")
    h = H // factor
    obs = torch.as_tensor(obs)
    if obs.dim() == 3:
        obs = obs[:, None]
    if tuple(obs.shape) != (n, 1, h, h):
        raise ValueError(f"obs must have shape {(n, 1, h, h)} (H / factor = {h}), got {tuple(obs.shape)}")
    if weight is None:
        weight = torch.ones(1, 1, h, h)
    weight = torch.as_tensor(weight)
    if weight.dim() == 3:
        weight = weight[:, None]
    if tuple(weight.shape) not in ((n, 1, h, h), (1, 1, h, h)):
        raise ValueError(f"weight must have shape {(n, 1, h, h)} or {(1, 1, h, h)}, got {tuple(weight.shape)}")
    if not (obs.is_floating_point() and weight.is_floating_point()):
        raise ValueError("obs and weight must be floating-point arrays")
    if not bool(((weight >= 0) & torch.isfinite(weight)).all()):          # NaN fails the comparison
        raise ValueError("weight values must be finite and >= 0")
    if not bool(torch.isfinite(obs)[(weight > 0).expand_as(obs)].all()):
        raise ValueError("obs holds a non-finite value where weight > 0")
    return obs, weight


def degrade(maps, factor: int, sigma: float = 0.0, seed: Optional[int] = None):
    """An observation of ``maps`` [n,1,H,H] (or [n,H,H]) as :class:`GuidedDDIMSampler` models one: the ``factor`` x
    ``factor`` block mean plus ``sigma`` times standard normal noise from a CPU generator seeded with ``seed`` (None: the
    global CPU RNG) -> [n,1,H/factor,H/factor] fp32 on the CPU.  A convenience on torch ops, not a kernel."""
    maps = torch.as_tensor(maps).detach().to("cpu", torch.float32)
    if maps.dim() == 3:
        maps = maps[:, None]
    if maps.dim() != 4 or maps.shape[1] != 1 or maps.shape[2] != maps.shape[3]:
        raise ValueError(f"maps must have shape [n, 1, H, H], got {tuple(maps.shape)}")
    if isinstance(factor, bool) or factor not in OBS_FACTORS or maps.shape[2] % factor != 0:
        raise ValueError(f"factor must be one of {OBS_FACTORS} and divide the map size {maps.shape[2]}, got {factor!r}")
    if not np.isfinite(sigma) or sigma < 0:
        raise ValueError(f"sigma must be finite and >= 0, got {sigma!r}")
    y = torch.nn.functional.avg_pool2d(maps, factor)
    if sigma > 0:
        g = None if seed is None else torch.Generator().manual_seed(int(seed))
        y = y + float(sigma) * torch.randn(y.shape, generator=g)
    return y


class GraphSampler:
    """One reverse-diffusion run (T steps) of ContextUnet on the HIP engine, hipGraph-replayed.

    Every sampler runs the one ``_step`` defined here: ``_prologue`` (device counter -> timestep, shortcut row), the eval
    forward, ``_update`` (the solver's kernel; here the reference's ancestral ``cdm_denoise``) and ``_blend``; and the one
    ``prepare_rng``, whose z draws follow the solver's ``_draws_host_z``.  A solver subclass overrides those two.

    Masked (inpainting) sampling, ``inpaint="fixed" | "fresh"`` with ``mask_n`` = n or 1 (the mask's batch extent):
    ``cdm_mask_blend`` follows the step kernel of every step, in the captured graph and in the eager tail, and
    re-imposes ``known`` where ``mask`` is 1 at the noise level of the state just written (:func:`known_tables`; the
    definition is in DESIGN §1).  ``run(x_T, known=, mask=)`` copies the two arrays into buffers allocated here once, so
    the captured graph serves any contents.  x_T itself is not blended.  The known-region noise xi is one draw for the run
    ("fixed") or one per step ("fresh"); with z_source="device" it is Philox in a key domain of its own, with "host" it
    comes from the CPU RNG: "fixed", one randn(n, 1, H, H) before the loop over the steps; "fresh", for i = T..2 one after
    that step's z and before its shortcut row(s) (the step to i = 0 needs none).  ``inpaint=None`` allocates and
    launches nothing new."""

    def __init__(self, model, sched: Schedule, n: int, guide_w: float, params: Optional[torch.Tensor],
                 save_rate: int = 20, z_source: str = "device", steps_per_graph: int = 10, seed: int = 1234,
                 snapshots: bool = True, use_graph: bool = True, positions: Optional[int] = None,
                 inpaint: Optional[str] = None, mask_n: Optional[int] = None):
        """``positions``: the number of steps of a run when it is not T (_StridedSampler); it sizes the per-step tables."""
        from .model import ContextUnet  # noqa: F401
        if inpaint is not None and inpaint not in KNOWN_NOISE_MODES:
            raise ValueError(f"inpaint must be None or one of {KNOWN_NOISE_MODES}, got {inpaint!r}")
        if inpaint is not None and model.in_channels != 1:
            raise ValueError(f"masked sampling is single-channel: the model has in_channels = {model.in_channels}")
        mask_n = n if mask_n is None else int(mask_n)
        if inpaint is not None and mask_n not in (1, n):
            raise ValueError(f"mask_n must be 1 or n = {n}, got {mask_n}")
        ktab = known_tables(sched.ab_t) if inpaint is not None else None    # validates before anything is allocated
        self.model, self.sched, self.n = model, sched, n
        self.T = sched.T
        self.npos = self.T if positions is None else int(positions)
        self.guide_w = float(guide_w)
        self.cfg = self.guide_w > 0 and params is not None
        self.z_source = z_source
        self.seed = seed
        eng, P = model._engine_and_params()
        self.eng, self.P = eng, P
        dev = P["out.3.weight"].device
        self.dev = dev
        H, nf, ncf = model.h, model.n_feat, model.n_cfeat
        self.H = H
        B = 2 * n if self.cfg else n
        self.B = B
        self.sets = 2 if self.cfg else 1
        self._repack()
        self.ws = self._workspace()
        E = lambda *sh: torch.empty(*sh, device=dev)
        self.xbuf = E(B, H, H)
        self.cbuf = torch.zeros(B, ncf, device=dev)
        if params is not None:
            self.cbuf[:n] = params.to(dev, torch.float32).reshape(n, ncf)
        self.has_c = params is not None
        self.t_cur = E(1)
        self.cur_i = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row = 2 * self.sets * nf
        self.sc_table = E(self.npos, self.row)
        self.sc_cur = E(self.row)
        slots, nslots = snapshot_slots(self.npos, save_rate)
        self.nslots = nslots if snapshots else 0
        self.slot = torch.from_numpy(slots).to(dev) if snapshots else None
        self.snaps = E(max(self.nslots, 1), n * H * H)
        self.z_table = E(max(self.npos - 1, 1), n * H * H) if self._needs_z_table() else None
        self.zseed = torch.zeros(1, dtype=torch.int64, device=dev)    # per-run Philox key (device z mode)
        self.K = max(1, int(steps_per_graph))
        self.use_graph = use_graph
        self.graph = None
        self.cur_k = self.steps_t = None                     # the ancestral form: position = timestep (cdm_mask_blend)
        self.inpaint, self.xi_table = inpaint, None
        if inpaint is not None:
            self.mask_n = mask_n
            self.known = torch.zeros(n * H * H, device=dev)
            self.mask = torch.zeros(mask_n * H * H, device=dev)
            self.ksab, self.ksomab = (torch.from_numpy(v).to(dev) for v in ktab)
            if z_source == "host":
                self.xi_table = E(1 if inpaint == "fixed" else max(self.npos - 1, 1), n * H * H)

    def _repack(self):
        """Refresh the weight pack the step's forward runs on (the eval pack, unless a subclass says otherwise)."""
        self.eng.repack(self.P, False, _s(), key=self.model._eval_pack_key(self.P))

    def _workspace(self):
        return self.eng.workspace(self.B, False)

    def _rehome(self, P):
        """The parameters moved to the tensors ``P``: the captured graph holds the old addresses."""
        self.P, self.graph = P, None

    def _draws_host_z(self, p: int) -> bool:
        """Whether position p of npos..1 takes a z from the CPU RNG in a host_z run (the solver's own rule)."""
        return p > 1

    def _needs_z_table(self):
        return self.z_source == "host" and any(self._draws_host_z(p) for p in range(1, self.npos + 1))

    def _lands_above_zero(self, p: int) -> bool:
        """Whether position p lands on a timestep >= 1 (the blend there needs a xi)."""
        return p > 1

    def _jumps(self, p: int) -> bool:
        """Whether the state is re-noised forward after position p (a position program, _StridedSampler)."""
        return False

    def _blend(self, s):
        """cdm_mask_blend on the state the step kernel has just written (no-op without inpainting)."""
        if self.inpaint is None:
            return
        numel = self.n * self.H * self.H
        lib().cdm_mask_blend(_p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(self.known), _p(self.mask),
                             self.mask.numel(), _p(self.cur_i), _p(self.cur_k), _p(self.steps_t), self.npos, self.T,
                             _p(self.ksab), _p(self.ksomab), _p(self.xi_table), numel,
                             1 if self.inpaint == "fresh" else 0, self.seed, _p(self.zseed), _p(self.slot),
                             _p(self.snaps), s)

    def prepare_rng(self, host_z: bool):
        """Draw the per-step CPU-RNG quantities in reference order, and with ``host_z`` z and the known-region xi too: the
        "fixed" xi, then for each position p = npos..1 z (where the solver draws one), the "fresh" xi (where the position
        lands on a timestep >= 1), the zeta of a position program's forward jump (where it jumps), the shortcut row(s).
        ValueError, nothing drawn: ``host_z`` on a sampler built without the host tables."""
        if host_z and self.z_source != "host":
            raise ValueError('prepare_rng(host_z=True) needs a sampler built with z_source="host"')
        draw = lambda: torch.randn(self.n, 1, self.H, self.H)
        if host_z and self.inpaint == "fixed":
            self.xi_table.copy_(draw().reshape(1, -1))
        rows, zs, xis = [], [], []
        for p in range(self.npos, 0, -1):
            if host_z and self._draws_host_z(p):
                zs.append(draw())
            if host_z and self.inpaint == "fresh" and self._lands_above_zero(p):
                xis.append(draw())
            if host_z and self._jumps(p):
                self.zeta_table[self.npos - p].copy_(draw().reshape(-1))
            rows.append(_draw_shortcut_row(self.model.n_feat, self.sets))
        self.sc_table.copy_(torch.stack(rows))
        for table, drawn in ((self.z_table, zs), (self.xi_table, xis)):
            if drawn:
                table.copy_(torch.stack(drawn).reshape(len(drawn), -1))

    # one step: prologue -> eval forward -> update (the part a solver defines) -> blend ------------------------------
    def _prologue(self, s):
        lib().cdm_sample_prologue(_p(self.ctr), self.T, _p(self.cur_i), _p(self.t_cur), _p(self.sc_table), self.row,
                                  _p(self.sc_cur), s)

    def _update(self, s, eps, numel):
        lib().cdm_denoise(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                          1 if self.cfg else 0, self.guide_w, _p(self.cur_i), _p(self.sched.coef), _p(self.sched.sa),
                          _p(self.sched.sb), _p(self.z_table), numel, self.seed, _p(self.zseed), _p(self.slot),
                          _p(self.snaps), self.T, s)

    def _step(self, s):
        self._prologue(s)
        half = self.sets * self.model.n_feat
        eps = self.eng.forward(self.ws, self.P, self.xbuf, self.t_cur, self.cbuf, self.sc_cur[:half], self.sc_cur[half:],
                               self.n, s)
        self._update(s, eps, self.n * self.H * self.H)
        self._blend(s)

    def _warm_up(self, s):
        self.ctr.fill_(self.npos)
        self._step(s)

    def prepare(self):
        """Refresh the weight pack and capture the step graph (idempotent)."""
        P = _rehomed(self.model, self.P)
        if P is not None:
            self._rehome(P)                                 # parameters were re-homed: re-capture
        self._repack()
        if self.use_graph and self.graph is None and self.npos >= self.K:
            self.graph = _capture_steps(self._warm_up, self._step, self.K)

    def run(self, x_T: torch.Tensor, steps: Optional[int] = None, known=None, mask=None):
        """Run every step (T of them; S for the strided sampler), or the first ``steps``, from x_T [n,1,H,H].
        A sampler built with ``inpaint`` takes ``known`` [n,1,H,H] and ``mask`` [mask_n,1,H,H] (both required, copied
        into its buffers; :func:`check_inpaint` is the caller's validation); any other takes neither.

        Returns (x [n,1,H,H], intermediate np [slots,n,1,H,H] or None)."""
        n, H = self.n, self.H
        if (known is None) != (mask is None) or (known is None) != (self.inpaint is None):
            raise ValueError("known= and mask= go together, with a sampler built with inpaint= and with no other")
        if known is not None:
            self.known.copy_(torch.as_tensor(known).to(self.dev, torch.float32).reshape(n * H * H))
            self.mask.copy_(torch.as_tensor(mask).to(self.dev, torch.float32).reshape(self.mask_n * H * H))
        if self.z_source == "device":
            # fresh z for every run, drawn from torch's CUDA generator (the reference's randn_like(x) on the device
            # consumes it too): reproducible under torch.cuda.manual_seed, different across consecutive calls.
            # Drawn before prepare(): a graph capture moves the generator's offset.
            self.zseed.random_()
        self.prepare()
        total = self.npos if steps is None else min(int(steps), self.npos)
        self.xbuf[:n] = x_T.to(self.dev, torch.float32).reshape(n, H, H)
        if self.cfg:
            self.xbuf[n:] = self.xbuf[:n]
        self.ctr.fill_(self.npos)
        _run_steps(self.graph, self._step, self.K, total)
        x = self.xbuf[:n].reshape(n, 1, H, H).clone()
        inter = None
        if self.nslots:
            inter = self.snaps[: self.nslots].reshape(self.nslots, n, 1, H, H).cpu().numpy()
        return x, inter


class _StridedSampler(GraphSampler):
    """GraphSampler over the subsequence ``taus`` (:func:`timestep_subsequence`) of the T timesteps: the device counter
    holds the position p = S..1 and ``cdm_sample_prologue_sub`` turns it into the timestep tau_p the network sees.  A
    solver subclass validates its tables before this constructor allocates anything, and defines ``_update`` and
    ``_draws_host_z``.  Snapshots follow the reference's rule on positions: ``snapshot_slots(S, save_rate)``.

    With a ``program`` (:func:`resample_program`: resampling jumps and / or a late start; None is the plain walk above,
    which launches exactly what it launched before programs existed) the run has P = program.P positions and everything
    sized or indexed by the position goes by P: the counter, the per-position tables of the solver, ``sc_table``, the z,
    zeta and xi tables, ``snapshot_slots(P, save_rate)``.  The prologue reads the program's ``from_t``; after the update,
    ``cdm_mask_blend_jump`` blends at the level ``land_t[p]`` (when the sampler has a mask) and re-noises the state
    forward where the position jumps, one launch for both; it is not launched when the program has neither a mask nor a
    jump (an unmasked late start).  Device noise is keyed by the position, each kind in a key domain of its own, so two
    visits to one timestep draw different z, xi and zeta.  Host zeta: one randn(n, 1, H, H) at each jumping position,
    after its z and "fresh" xi and before its shortcut row(s)."""

    def __init__(self, model, sched, n, guide_w, params, taus, save_rate, z_source, steps_per_graph, seed, snapshots,
                 use_graph, inpaint, mask_n, program: Optional[Program] = None):
        self.taus, self.S = taus, len(taus)
        self.program = program
        if program is not None and model.in_channels != 1:
            raise ValueError("resampling and late start are single-channel, like masked sampling: the model has "
                             f"in_channels = {model.in_channels}")
        if program is not None and program.P > sched.T:
            raise ValueError(f"the program has {program.P} positions, more than the T = {sched.T} timesteps the step "
                             "prologue serves: lower resample, raise jump or take fewer steps")
        super().__init__(model, sched, n, guide_w, params, save_rate, z_source, steps_per_graph, seed, snapshots,
                         use_graph, positions=self.S if program is None else program.P, inpaint=inpaint, mask_n=mask_n)
        self.cur_k = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.zeta_table = None
        if program is None:
            self.steps_t = torch.tensor([0] + self.taus, dtype=torch.int32, device=self.dev)
            return
        dv = lambda v: torch.from_numpy(v).to(self.dev)       # noqa: E731
        self.steps_t, self.land_t, self.fa, self.fb = dv(program.from_t), dv(program.land_t), dv(program.fa), dv(program.fb)
        self.any_jump = bool((program.up_t != program.land_t).any())
        if self.any_jump and z_source == "host":
            self.zeta_table = torch.zeros(max(self.npos - 1, 1), n * self.H * self.H, device=self.dev)

    def _lands_above_zero(self, p):
        return p > 1 if self.program is None else int(self.program.land_t[p]) >= 1

    def _jumps(self, p):
        return self.program is not None and int(self.program.up_t[p]) != int(self.program.land_t[p])

    def _prologue(self, s):
        lib().cdm_sample_prologue_sub(_p(self.ctr), self.npos, self.T, _p(self.steps_t), _p(self.cur_i), _p(self.cur_k),
                                      _p(self.t_cur), _p(self.sc_table), self.row, _p(self.sc_cur), s)

    def _blend(self, s):
        if self.program is None:
            return super()._blend(s)
        if self.inpaint is None and not self.any_jump:
            return
        numel = self.n * self.H * self.H
        ip = self.inpaint is not None
        lib().cdm_mask_blend_jump(_p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel,
                                  _p(self.known) if ip else None, _p(self.mask) if ip else None,
                                  self.mask.numel() if ip else 0, _p(self.cur_k), _p(self.land_t), self.npos, self.T,
                                  _p(self.ksab) if ip else None, _p(self.ksomab) if ip else None, _p(self.fa),
                                  _p(self.fb), _p(self.xi_table), numel, 1 if self.inpaint == "fresh" else 0,
                                  _p(self.zeta_table), numel, self.seed, _p(self.zseed), _p(self.slot), _p(self.snaps), s)


class DDIMSampler(_StridedSampler):
    """Strided reverse diffusion: S of the T timesteps (:func:`timestep_subsequence`) with the update of
    :func:`ddim_tables`, on GraphSampler's buffers, RNG modes, snapshots and captured step graph.

    At the position p = S..1 (:class:`_StridedSampler`) ``cdm_ddim_step`` applies
    x <- (cx[p] x + ce[p] eps) + sigma[p] z.  CPU-RNG order (z_source="host"), for
    p = S..1: z (only when eta > 0 and p > 1), then the shortcut row(s), cond before uncond; eta = 0 draws no z at all.
    In "device" mode z is Philox stream tau_p of the per-run key, as the full sampler's stream i.

    Masked sampling (``inpaint``, ``mask_n``: see :class:`GraphSampler`) blends after every position, at the noise level
    of tau_{p-1}.  Host xi: "fixed", one randn(n, 1, H, H) before the loop over the positions; "fresh", for p = S..2 one
    after that position's z (if any) and before its shortcut row(s).

    ``resample`` / ``jump`` / ``t_start`` other than 1 / 1 / None run the position program of :func:`resample_program`
    (:class:`_StridedSampler`): tables from :func:`ddim_tables_from_pairs`, and ``cdm_ddim_step_pos``, whose device z is
    keyed by the position, since a program visits one timestep more than once."""

    def __init__(self, model, sched: Schedule, n: int, guide_w: float, params: Optional[torch.Tensor],
                 steps=50, eta: float = 0.0, spacing="uniform", save_rate: int = 20, z_source: str = "device",
                 steps_per_graph: int = 10, seed: int = 1234, snapshots: bool = True, use_graph: bool = True,
                 inpaint: Optional[str] = None, mask_n: Optional[int] = None, resample: int = 1, jump: int = 1,
                 t_start: Optional[int] = None):
        taus = timestep_subsequence(sched.T, steps, spacing)
        self.eta = float(eta)
        prog = _program(sched.ab_t, taus, resample, jump, t_start, inpaint)
        if prog is None:
            tables = ddim_tables(sched.ab_t, taus, self.eta)               # validates eta before anything is allocated
        else:
            tables = ddim_tables_from_pairs(sched.ab_t, prog.from_t, prog.land_t, self.eta)
        super().__init__(model, sched, n, guide_w, params, taus, save_rate, z_source, steps_per_graph, seed, snapshots,
                         use_graph, inpaint, mask_n, prog)
        self.cx, self.ce, self.sigma = (torch.from_numpy(v).to(self.dev) for v in tables)

    def _draws_host_z(self, p):
        return self.eta > 0 and p > 1

    def _update(self, s, eps, numel):
        if self.program is not None:                         # z keyed by the position: a timestep may be visited twice
            lib().cdm_ddim_step_pos(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                                    1 if self.cfg else 0, self.guide_w, _p(self.cur_k), _p(self.cx), _p(self.ce),
                                    _p(self.sigma), self.npos, _p(self.z_table), numel, self.seed, _p(self.zseed),
                                    _p(self.slot), _p(self.snaps), s)
            return
        lib().cdm_ddim_step(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                            1 if self.cfg else 0, self.guide_w, _p(self.cur_i), _p(self.cur_k), _p(self.cx), _p(self.ce),
                            _p(self.sigma), self.S, _p(self.z_table), numel, self.seed, _p(self.zseed), _p(self.slot),
                            _p(self.snaps), s)


class DPMSolverSampler(_StridedSampler):
    """Strided reverse diffusion with the multistep update of :func:`dpmpp_tables` (DPM-Solver++ 2M; ``order=1`` is DDIM
    at eta = 0 written on the data prediction), on GraphSampler's buffers, snapshots and captured step graph.

    At the position p = S..1 (:class:`_StridedSampler`) ``cdm_dpmpp_step`` applies the update and keeps the previous
    data prediction in ``dprev``, allocated here
    once so a captured graph stays valid across runs (its stale contents are never read: c1 = 0 at the first position).
    The solver is deterministic: no z in any ``z_source``.  CPU-RNG order, for p = S..1: the shortcut row(s), cond
    before uncond, and nothing else.

    Masked sampling (``inpaint``, ``mask_n``: see :class:`GraphSampler`) blends after every position, at the noise level
    of tau_{p-1}; ``dprev`` keeps the data prediction computed before the blend (from the state the network saw), the
    blended state enters the next position as x_i.  Use "fixed": noise re-drawn at every step ("fresh") breaks the
    smoothness along the trajectory that the second-order combination relies on.  The known-region xi is the one
    quantity that depends on ``z_source`` here.  Host xi: "fixed", one randn(n, 1, H, H) before the loop over the
    positions; "fresh", for p = S..2 one before that position's shortcut row(s).

    ``resample`` / ``jump`` / ``t_start`` other than 1 / 1 / None run the position program of :func:`resample_program`
    (:class:`_StridedSampler`) with the tables of :func:`dpmpp_tables_from_pairs`: the position after a forward jump is
    first order (c1 = 0, ``dprev`` not read), as the first one is."""

    def __init__(self, model, sched: Schedule, n: int, guide_w: float, params: Optional[torch.Tensor],
                 steps=20, order: int = 2, spacing="uniform", save_rate: int = 20, z_source: str = "device",
                 steps_per_graph: int = 10, seed: int = 1234, snapshots: bool = True, use_graph: bool = True,
                 inpaint: Optional[str] = None, mask_n: Optional[int] = None, resample: int = 1, jump: int = 1,
                 t_start: Optional[int] = None):
        taus = timestep_subsequence(sched.T, steps, spacing)
        prog = _program(sched.ab_t, taus, resample, jump, t_start, inpaint)
        if prog is None:
            tables = dpmpp_tables(sched.ab_t, taus, order)                # validates order before anything is allocated
        else:                                                # the history is dropped after a jump: c1 = 0 there
            tables = dpmpp_tables_from_pairs(sched.ab_t, prog.from_t, prog.land_t, prog.up_t, order)
        self.order = int(order)
        super().__init__(model, sched, n, guide_w, params, taus, save_rate, z_source, steps_per_graph, seed, snapshots,
                         use_graph, inpaint, mask_n, prog)
        self.tables = tuple(torch.from_numpy(v).to(self.dev) for v in tables)  # sq, ra, c0, c1, cx, cd
        self.dprev = torch.empty(n * self.H * self.H, device=self.dev)

    def _draws_host_z(self, p):
        return False

    def _update(self, s, eps, numel):
        lib().cdm_dpmpp_step(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                             1 if self.cfg else 0, self.guide_w, _p(self.cur_k), *(_p(t) for t in self.tables), self.npos,
                             _p(self.dprev), _p(self.slot), _p(self.snaps), s)


class GuidedDDIMSampler(_StridedSampler):
    """Strided DDIM sampling guided by a coarse, noisy, partly missing observation (diffusion posterior sampling, Chung
    et al. 2023; not in the reference; DESIGN §1 has the definition).

    Observation model y = A x0 + n: A the f x f block mean [H, H] -> [H / f, H / f], ``weight`` [n or 1, H / f, H / f] a
    relative inverse variance per cell, 0 = not observed.  At the position p = S..1 of the plain walk over ``taus``:
        eps    = the frozen train-structured forward (model.eval()'s forward kept for a backward), CFG-combined
        x0h    = (x - sq[p] eps) ra[p];   r = y - A x0h;   L[s] = sum_q wgt_q r_q^2          (``cdm_obs_residual_grad``)
        grad   = dL/dx = A^T-term through x0h directly + the engine's full backward of dL/d eps (``dx=``)
        x     <- DDIM step of p - (zeta / (2 sqrt(L[s]))) grad                               (``cdm_ddim_step_guided``)
    a step of length ``zeta`` down the gradient of the misfit norm sqrt(L) after every DDIM step.  ``zeta`` = 0 launches
    neither the backward nor the gradient outputs and is the DDIM step bit for bit; L is still recorded.  ``hist``
    [S + 1, n] fp64 keeps L by position (row p).

    The sampler runs on the engine's train pack and a frozen workspace ``eng.workspace(B, True, frozen=True)``, which
    keeps the fp32 activations of all B rows for the backward: n is bounded by memory.  As :class:`ParamFit` does, it
    renews the pack token and invalidates the model's eval pack, so a Trainer, an autograd backward or an eval call
    sharing the engine afterwards repacks its own weights.  ``run(x_T, obs=, weight=)`` copies the two arrays into
    buffers allocated here once, so the captured graph serves any contents.  Device z is keyed by the position, in
    ``cdm_ddim_step_pos``'s key domain; the host z table goes by row S - p.  CPU-RNG order: :class:`DDIMSampler`'s."""

    def __init__(self, model, sched: Schedule, n: int, guide_w: float, params: Optional[torch.Tensor],
                 steps=50, eta: float = 0.0, spacing="uniform", save_rate: int = 20, z_source: str = "device",
                 steps_per_graph: int = 10, seed: int = 1234, snapshots: bool = True, use_graph: bool = True,
                 factor: int = 4, weight_n: int = 1, zeta: float = 1.0):
        taus = timestep_subsequence(sched.T, steps, spacing)
        self.eta, self.zeta, self.factor = float(eta), float(zeta), int(factor)
        tables = ddim_tables(sched.ab_t, taus, self.eta)                   # validates before anything is allocated
        gtab = guided_tables(sched.ab_t, taus)
        H = model.h
        if isinstance(factor, bool) or factor not in OBS_FACTORS or H % factor != 0:
            raise ValueError(f"factor must be one of {OBS_FACTORS} and divide the map size {H}, got {factor!r}")
        if not np.isfinite(self.zeta) or self.zeta < 0:
            raise ValueError(f"zeta must be finite and >= 0, got {zeta!r}")
        if weight_n not in (1, n):
            raise ValueError(f"weight_n must be 1 or n = {n}, got {weight_n}")
        if model.in_channels != 1:
            raise ValueError(f"observation-guided sampling is single-channel: the model has in_channels = "
                             f"{model.in_channels}")
        super().__init__(model, sched, n, guide_w, params, taus, save_rate, z_source, steps_per_graph, seed, snapshots,
                         use_graph, None, None, None)
        dev, B = self.dev, self.B
        self.K = min(self.K, self.npos)                      # a short walk is one graph
        self.cx, self.ce, self.sigma = (torch.from_numpy(v).to(dev) for v in tables)
        self.sq, self.ra = (torch.from_numpy(v).to(dev) for v in gtab)
        cells = (H // self.factor) ** 2
        self.weight_n = int(weight_n)
        self.obs = torch.zeros(n * cells, device=dev)
        self.wgt = torch.zeros(self.weight_n * cells, device=dev)
        self.L = torch.zeros(n, dtype=torch.float64, device=dev)
        self.hist = torch.zeros(self.npos + 1, n, dtype=torch.float64, device=dev)
        # the closing misfit of the final x itself: x0h = x (tables sq = 0, ra = 1 of a one-position walk)
        self.one = torch.ones(1, dtype=torch.int32, device=dev)
        self.sq0, self.ra1 = torch.zeros(2, device=dev), torch.ones(2, device=dev)
        self.last = torch.zeros(2, n, dtype=torch.float64, device=dev)
        self.deps = self.gdir = self.dx = None
        if self.zeta > 0:
            self.deps, self.gdir, self.dx = (torch.empty(B, H, H, device=dev), torch.empty(n, H, H, device=dev),
                                             torch.empty(B, H, H, device=dev))
        self._rehome(self.P)

    def _repack(self):
        self.eng.repack(self.P, True, _s())
        self.eng.train_pack_token = object()
        self.model._invalidate_eval_pack()

    def _workspace(self):
        return self.eng.workspace(self.B, True, frozen=True)

    def _rehome(self, P):
        super()._rehome(P)
        # scratch parameter gradients of the backward (written, never read)
        self.G = {k: torch.empty_like(P[k]) for k in self.model._param_names} if self.zeta > 0 else None

    def _draws_host_z(self, p):
        return self.eta > 0 and p > 1

    def _residual(self, s, x, eps, cfg, cur_k, sq, ra, npos, hist, deps, gdir):
        lib().cdm_obs_residual_grad(_p(x), _p(eps), 1 if cfg else 0, self.guide_w, _p(self.obs), _p(self.wgt),
                                    self.wgt.numel(), self.n, self.H, self.factor, _p(cur_k), _p(sq), _p(ra), npos,
                                    _p(self.L), _p(hist), _p(deps), _p(gdir), s)

    def _step(self, s):
        self._prologue(s)
        half = self.sets * self.model.n_feat
        eps = self.eng.forward(self.ws, self.P, self.xbuf, self.t_cur, self.cbuf, self.sc_cur[:half], self.sc_cur[half:],
                               self.n, s, frozen=True)
        self._residual(s, self.xbuf, eps, self.cfg, self.cur_k, self.sq, self.ra, self.npos, self.hist, self.deps,
                       self.gdir)
        if self.zeta > 0:
            self.eng.backward(self.ws, self.P, self.deps, self.G, s, dx=self.dx)
        numel = self.n * self.H * self.H
        lib().cdm_ddim_step_guided(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                                   1 if self.cfg else 0, self.guide_w, _p(self.cur_k), _p(self.cx), _p(self.ce),
                                   _p(self.sigma), self.npos, _p(self.z_table), numel, self.seed, _p(self.zseed),
                                   _p(self.slot), _p(self.snaps), _p(self.gdir), _p(self.dx), _p(self.L), self.zeta,
                                   self.H, s)

    def run(self, x_T: torch.Tensor, steps: Optional[int] = None, obs=None, weight=None):
        """Every position (or the first ``steps``) from x_T [n,1,H,H] under the observation ``obs`` [n,1,h,h] and
        ``weight`` [weight_n,1,h,h] (both required, copied into this sampler's buffers; :func:`check_observation` is the
        caller's validation) -> (x [n,1,H,H], intermediate np [slots,n,1,H,H] or None, misfit [S + 1, n] fp64 on the
        host): misfit[S - p] = sqrt(L) seen at position p, the last row sqrt(L) of the final x itself."""
        if obs is None or weight is None:
            raise ValueError("a guided sampler needs obs= and weight=")
        self.obs.copy_(torch.as_tensor(obs).to(self.dev, torch.float32).reshape(-1))
        self.wgt.copy_(torch.as_tensor(weight).to(self.dev, torch.float32).reshape(-1))
        self.hist.zero_()
        x, inter = super().run(x_T, steps)
        self._residual(_s(), self.xbuf, self.xbuf, False, self.one, self.sq0, self.ra1, 1, self.last, None, None)
        L = torch.cat([self.hist[1:].flip(0), self.last[1:]])
        return x, inter, L.sqrt().cpu()


class DDIMEncoder(_StridedSampler):
    """DDIM inversion: the ascending walk of :func:`encode_tables` from a map x_0 to its latent x_T on the eval forward
    (no backward), on GraphSampler's buffers, snapshots and captured step graph.  Not in the reference.

    At the position p = S..1 the prologue hands the network the timestep from_t[p] = tau_{S+1-p} and the unchanged
    ``cdm_ddim_step_pos`` applies x <- ix[p] x + ie[p] eps with the tables (ix, ie, 0): the encoder needs no kernel of
    its own.  CFG (``guide_w`` > 0 with params) combines eps as the samplers do.  Nothing is random but the shortcut
    row(s) of every forward, drawn from the CPU RNG for p = S..1, cond before uncond (``prepare_rng``); decoding with
    ``sample_ddim_from_noise(eta=0)`` draws its own, so a round trip is exact only up to those and the discretisation.
    Snapshots: ``snapshot_slots(S, save_rate)`` on positions, the last one the latent."""

    def __init__(self, model, sched: Schedule, n: int, guide_w: float, params: Optional[torch.Tensor], steps=50,
                 spacing="uniform", save_rate: int = 20, steps_per_graph: int = 10, seed: int = 1234,
                 snapshots: bool = True, use_graph: bool = True):
        taus = timestep_subsequence(sched.T, steps, spacing)
        tables = encode_tables(sched.ab_t, taus)              # validates before anything is allocated
        if model.in_channels != 1:
            raise ValueError(f"encoding is single-channel, like the samplers: the model has in_channels = "
                             f"{model.in_channels}")
        super().__init__(model, sched, n, guide_w, params, taus, save_rate, "device", steps_per_graph, seed, snapshots,
                         use_graph, None, None, None)
        self.K = min(self.K, self.npos)                      # a short walk is one graph
        self.steps_t, self.ix, self.ie = (torch.from_numpy(v).to(self.dev) for v in tables[:3])
        self.sigma0 = torch.zeros(self.npos + 1, device=self.dev)

    def _draws_host_z(self, p):
        return False

    def _update(self, s, eps, numel):
        lib().cdm_ddim_step_pos(_p(self.xbuf), _p(self.xbuf), _p(self.xbuf) if self.cfg else None, numel, _p(eps),
                                1 if self.cfg else 0, self.guide_w, _p(self.cur_k), _p(self.ix), _p(self.ie),
                                _p(self.sigma0), self.npos, None, numel, self.seed, _p(self.zseed), _p(self.slot),
                                _p(self.snaps), s)


class FlowLikelihood(_StridedSampler):
    """The log-density of the eta = 0 DDIM sampler's model by the change of variables along the probability-flow ODE
    (Song et al. 2021, §4.3 and App. D.2; not in the reference; DESIGN §1 has the definition).

    At the position p = S..1 of the ascending walk (:func:`encode_tables`), all on the captured step graph and with
    nothing read back between positions:
        eps  = the frozen train-structured forward at the timestep from_t[p] (model.eval()'s forward kept for a backward)
        v    = the Rademacher probe of the position, written into deps                         (``cdm_flow_probe``)
        dx   = J^T v, the engine's full backward with ``dx=``
        q    = <dx, v>;  acc += ld(g[p] q);  x <- ix[p] x + ie[p] eps                         (``cdm_flow_step``)
    and after the walk ``cdm_flow_finish`` adds log N(x_T; 0, I) + (D / 2) log ab_T.  ``form``: "trace", ld = g q, or
    "logdet", ld = D log1p(g q / D).  The probe is keyed by position and element, not by the row: all maps of a run
    share their probes (the scan's common random numbers).  ``run(x_0, n_probe=R, seed=)`` replays the same graph R
    times with the run keys :func:`flow_run_key` (seed, r), r = 0..R-1, handed to the kernels through a device value, so
    one sampler and one captured graph serve every seed; the shortcut rows are whatever ``prepare_rng`` drew last and
    stay the same for every probe run, so all probes see one function.

    Like :class:`GuidedDDIMSampler` it runs on the engine's train pack and a frozen workspace (fp32 activations of all
    n rows: n is bounded by memory), renews the pack token and invalidates the model's eval pack.  The parameter
    gradients the backward also computes go to scratch and are wasted work.  ValueError before anything is allocated:
    ``guide_w`` != 0, in_channels > 1, an unknown ``form``, what :func:`encode_tables` raises."""

    def __init__(self, model, sched: Schedule, n: int, params: Optional[torch.Tensor], steps=50, spacing="uniform",
                 form: str = "logdet", steps_per_graph: int = 10, seed: int = 1234, use_graph: bool = True,
                 guide_w: float = 0.0):
        taus = timestep_subsequence(sched.T, steps, spacing)
        tables = encode_tables(sched.ab_t, taus)              # validates before anything is allocated
        if not float(guide_w) == 0.0:
            raise ValueError(f"the flow likelihood is the unguided sampler's density: guide_w must be 0, got {guide_w!r}")
        if model.in_channels != 1:
            raise ValueError(f"the flow likelihood is single-channel: the model has in_channels = {model.in_channels}")
        if form not in FLOW_FORMS:
            raise ValueError(f"form must be one of {FLOW_FORMS}, got {form!r}")
        self.form, self.run_seed = form, int(seed)
        # the kernels' by-value seed is 0: the whole run key travels in zseed
        super().__init__(model, sched, n, 0.0, params, taus, 20, "device", steps_per_graph, 0, False, use_graph, None,
                         None, None)
        dev, H = self.dev, self.H
        self.K = min(self.K, self.npos)                      # a short walk is one graph
        self.steps_t, self.ix, self.ie, self.g = (torch.from_numpy(v).to(dev) for v in tables)
        self.log_abT = float(np.log(_ab64(sched.ab_t)[sched.T]))
        self.deps, self.dx = torch.empty(n, H, H, device=dev), torch.empty(n, H, H, device=dev)
        F64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)    # noqa: E731
        self.acc, self.prior, self.logp, self.hist = F64(n), F64(n), F64(n), F64(self.npos + 1, n)
        self.invalid = torch.zeros(n, dtype=torch.int32, device=dev)
        self._rehome(self.P)

    def _repack(self):
        self.eng.repack(self.P, True, _s())
        self.eng.train_pack_token = object()
        self.model._invalidate_eval_pack()

    def _workspace(self):
        return self.eng.workspace(self.B, True, frozen=True)

    def _rehome(self, P):
        super()._rehome(P)
        self.G = {k: torch.empty_like(P[k]) for k in self.model._param_names}   # scratch: written, never read

    def _draws_host_z(self, p):
        return False

    def _step(self, s):
        self._prologue(s)
        nf = self.model.n_feat
        eps = self.eng.forward(self.ws, self.P, self.xbuf, self.t_cur, self.cbuf, self.sc_cur[:nf], self.sc_cur[nf:],
                               self.n, s, frozen=True)
        lb = lib()
        lb.cdm_flow_probe(_p(self.deps), self.n, self.H, _p(self.cur_k), self.npos, 0, _p(self.zseed), s)
        self.eng.backward(self.ws, self.P, self.deps, self.G, s, dx=self.dx)
        lb.cdm_flow_step(_p(self.xbuf), _p(eps), _p(self.dx), self.n, self.H, _p(self.cur_k), _p(self.ix), _p(self.ie),
                         _p(self.g), self.npos, FLOW_FORMS.index(self.form), 0, _p(self.zseed), _p(self.acc),
                         _p(self.hist), _p(self.invalid), s)

    def run(self, x_0: torch.Tensor, n_probe: int = 1, steps: Optional[int] = None, seed: Optional[int] = None):
        """``n_probe`` runs of the walk (or of its first ``steps`` positions) from the maps x_0 [n,1,H,H], run r under
        the key flow_run_key(seed, r) (``seed`` None: the constructor's) -> dict of host tensors: logp [R, n], prior
        [R, n], acc [R, n] (sum_k ld_k), hist [R, S, n] (q_k in step order), invalid [n] bool, latent [n,1,H,H] fp32."""
        n, H = self.n, self.H
        R = _posint("n_probe", n_probe)
        seed = self.run_seed if seed is None else int(seed)
        self.prepare()
        total = self.npos if steps is None else min(int(steps), self.npos)
        x0 = x_0.to(self.dev, torch.float32).reshape(n, H, H)
        self.invalid.zero_()
        out = dict(logp=[], prior=[], acc=[], hist=[])
        for r in range(R):
            key = flow_run_key(seed, r)
            self.zseed.fill_(key - (1 << 64) if key >> 63 else key)      # the same 64 bits as a signed value
            self.acc.zero_(); self.hist.zero_()
            self.xbuf.copy_(x0)
            self.ctr.fill_(self.npos)
            _run_steps(self.graph, self._step, self.K, total)
            lib().cdm_flow_finish(_p(self.xbuf), n, H, self.log_abT, _p(self.acc), _p(self.prior), _p(self.logp), _s())
            out["logp"].append(self.logp.cpu()); out["prior"].append(self.prior.cpu()); out["acc"].append(self.acc.cpu())
            out["hist"].append(self.hist[1:].flip(0).cpu())
        res = {k: torch.stack(v) for k, v in out.items()}
        res["invalid"] = self.invalid.cpu() != 0
        res["latent"] = self.xbuf.reshape(n, 1, H, H).cpu()
        res["log_abT"] = self.log_abT
        return res


PLAIN = (1, 1, None)          # (resample, jump, t_start) of the plain walk: no position program


class DDPM:
    """Script-globals bundle of the reference (nn_model, timesteps, b_t/a_t/ab_t, n_cfeat, device)."""

    def __init__(self, model, timesteps: int, device="cuda", z_source: str = "device", seed: int = 1234,
                 sched_tensors=None, sched_sb=None):
        """sched_tensors = (b_t, a_t, ab_t) and sched_sb = the b_t.sqrt() table to use (Schedule); None: built here."""
        self.model, self.T = model, int(timesteps)
        self.sched = Schedule(self.T, device, tensors=sched_tensors, sb=sched_sb)
        self.b_t, self.a_t, self.ab_t = self.sched.tensors()
        self.device = torch.device(device)
        self.n_cfeat = model.n_cfeat
        self.z_source = z_source
        self.seed = seed
        self._samplers = {}

    def perturb_input(self, x, t, noise):
        return perturb_input(x, t, noise, self.sched)

    def denoise_add_noise(self, x, t, pred_noise, z=None):
        return denoise_add_noise(x, t, pred_noise, z, self.sched)

    def _sampler(self, n, guide_w, params, save_rate, solver=None, inpaint=None, prog=PLAIN):
        """The cached sampler of a configuration.  ``solver``: None, the ancestral GraphSampler, or (sampler class, steps,
        eta or order, spacing) of a strided one; ``inpaint = (known_noise, mask batch extent)`` the masked form of any of
        them (a trailing tagged entry of the key: the contents of known / mask are not part of it, one sampler and one
        captured graph serve them all); ``prog = (resample, jump, t_start)`` of a strided one, a further tagged entry
        unless it is the plain walk (1, 1, None), whose key and sampler are those of a call without the three."""
        key = (n, float(guide_w) if params is not None else 0.0, params is not None, save_rate, self.z_source)
        cls, sargs = GraphSampler, ()
        if solver is not None:
            cls, steps, opt, spacing = solver
            sargs = (steps, opt, spacing)
            key += (cls, steps, opt, spacing if isinstance(spacing, str) else tuple(spacing))
        ip = {}
        if inpaint is not None:
            key += (("inpaint",) + tuple(inpaint),)
            ip = dict(inpaint=inpaint[0], mask_n=inpaint[1])
        if tuple(prog) != PLAIN:
            key += (("program",) + tuple(prog),)
            ip.update(resample=prog[0], jump=prog[1], t_start=prog[2])
        smp = self._samplers.get(key)
        if smp is None:
            smp = self._samplers[key] = cls(self.model, self.sched, n, guide_w, params, *sargs, save_rate, self.z_source,
                                            seed=self.seed, **ip)
        elif params is not None:
            smp.cbuf[:n] = params.to(smp.dev, torch.float32).reshape(n, -1)
        return smp

    @torch.no_grad()
    def _sample(self, solver, x_T, size, params, guide_w, save_rate, known, mask, known_noise, prog=PLAIN):
        """Every sample_* method.  ``x_T``: the noise images, or their number to draw them [n,1,size,size], and random
        ``params`` when none are given, from the CPU RNG as the reference does.  The masked-sampling inputs are validated
        before anything is drawn, so a ValueError leaves the CPU RNG where it was; so is ``prog`` = (resample, jump,
        t_start), the position program of a strided sampler (:func:`resample_program`)."""
        draw = not torch.is_tensor(x_T)
        assert not draw or size == self.model.h
        n = x_T if draw else x_T.shape[0]
        known, mask = check_inpaint(known, mask, n, self.model.h, known_noise, self.model.in_channels)
        if tuple(prog) != PLAIN:
            if solver is None:
                raise ValueError('resample, jump and t_start need a strided sampler: the ancestral one has no position '
                                 'program; its update is sampler="ddim", eta=1.0 on all T steps')
            if self.model.in_channels != 1:
                raise ValueError("resampling and late start are single-channel, like masked sampling: the model has "
                                 f"in_channels = {self.model.in_channels}")
            _program(self.sched.ab_t, timestep_subsequence(self.T, solver[1], solver[3]), *prog,
                     None if known is None else known_noise)
        if draw:
            x_T = torch.randn(n, 1, size, size)
            if params is None:
                params = torch.rand(n, self.n_cfeat)
        smp = self._sampler(n, guide_w, params, save_rate, solver,
                            None if known is None else (known_noise, int(mask.shape[0])), prog)
        smp.prepare_rng(host_z=self.z_source == "host")
        return smp.run(x_T, known=known, mask=mask)

    def sample_ddpm(self, n_sample=1, size=64, device=None, params=None, guide_w=0.0, save_rate=20, *, known=None,
                    mask=None, known_noise="fixed"):
        """code/train_diffusion_condition.py:281-335 -> (samples, intermediate).  ``known`` [n,1,size,size] and ``mask``
        [n or 1,1,size,size] (keyword only, both or neither; 1 = known pixel, 0 = generated, between: a soft blend) run
        masked sampling with the known-region noise mode ``known_noise`` ("fixed" | "fresh", :class:`GraphSampler`);
        :func:`check_inpaint` lists what raises ValueError."""
        return self._sample(None, n_sample, size, params, guide_w, save_rate, known, mask, known_noise)

    def sample_ddpm_from_noise(self, noise_images, params=None, save_rate=20, guide_w=0.0, *, known=None, mask=None,
                               known_noise="fixed"):
        """code/train_diffusion_condition.py:337-384 (and the unconditional code/train_diffusion.py:170-193).
        ``known`` / ``mask`` / ``known_noise``: masked sampling, as in :meth:`sample_ddpm` (noise_images is not blended)."""
        return self._sample(None, noise_images, None, params, guide_w, save_rate, known, mask, known_noise)

    def sample_ddim(self, n_sample=1, size=64, device=None, params=None, guide_w=0.0, steps=50, eta=0.0,
                    spacing="uniform", save_rate=20, *, known=None, mask=None, known_noise="fixed", resample=1, jump=1,
                    t_start=None):
        """sample_ddpm on ``steps`` of the T timesteps (:class:`DDIMSampler`; ``spacing``: "uniform", "quadratic" or an
        explicit increasing timestep list ending at T, then ``steps`` may be None) -> (samples, intermediate).  x_T and
        random params consume the CPU RNG as sample_ddpm does; eta = 0 is deterministic given x_T and the shortcut
        draws, eta = 1 has the ancestral sampler's variance.  Snapshots: snapshot_slots(steps, save_rate) on positions.
        ``known`` / ``mask`` / ``known_noise``: masked sampling, as in :meth:`sample_ddpm`.  ``resample`` = R, ``jump`` = J
        and ``t_start`` (keyword only) run the position program of :func:`resample_program` instead of the plain walk:
        RePaint's resampling (R > 1 needs known / mask; the run then makes (R - 1) J (S' // J - 1) more network
        evaluations) and / or a start from the largest timestep <= t_start, where the first argument is the state at that
        level (:meth:`refine` builds one); snapshots then go by snapshot_slots(P, save_rate).  All three at their
        defaults is the call without them."""
        return self._sample((DDIMSampler, steps, float(eta), spacing), n_sample, size, params, guide_w, save_rate, known,
                            mask, known_noise, (resample, jump, t_start))

    def sample_ddim_from_noise(self, noise_images, params=None, steps=50, eta=0.0, spacing="uniform", save_rate=20,
                               guide_w=0.0, *, known=None, mask=None, known_noise="fixed", resample=1, jump=1,
                               t_start=None):
        """sample_ddpm_from_noise on ``steps`` of the T timesteps (see :meth:`sample_ddim`)."""
        return self._sample((DDIMSampler, steps, float(eta), spacing), noise_images, None, params, guide_w, save_rate,
                            known, mask, known_noise, (resample, jump, t_start))

    def sample_dpm(self, n_sample=1, size=64, device=None, params=None, guide_w=0.0, steps=20, order=2,
                   spacing="uniform", save_rate=20, *, known=None, mask=None, known_noise="fixed", resample=1, jump=1,
                   t_start=None):
        """sample_ddpm on ``steps`` of the T timesteps with the second-order multistep update (:class:`DPMSolverSampler`;
        ``order=1``: first order throughout; ``spacing`` as in :meth:`sample_ddim`) -> (samples, intermediate).  x_T and
        random params consume the CPU RNG as sample_ddpm does; the run is deterministic given x_T and the shortcut
        draws.  Snapshots: snapshot_slots(steps, save_rate) on positions.  ``known`` / ``mask`` / ``known_noise``:
        masked sampling, as in :meth:`sample_ddpm` (keep "fixed" here, see :class:`DPMSolverSampler`).  ``resample`` /
        ``jump`` / ``t_start``: the position program, as in :meth:`sample_ddim`; the multistep history is dropped after
        every jump (:func:`dpmpp_tables_from_pairs`)."""
        return self._sample((DPMSolverSampler, steps, order, spacing), n_sample, size, params, guide_w, save_rate, known,
                            mask, known_noise, (resample, jump, t_start))

    def sample_dpm_from_noise(self, noise_images, params=None, steps=20, order=2, spacing="uniform", save_rate=20,
                              guide_w=0.0, *, known=None, mask=None, known_noise="fixed", resample=1, jump=1,
                              t_start=None):
        """sample_ddpm_from_noise on ``steps`` of the T timesteps (see :meth:`sample_dpm`)."""
        return self._sample((DPMSolverSampler, steps, order, spacing), noise_images, None, params, guide_w, save_rate,
                            known, mask, known_noise, (resample, jump, t_start))

    def inpaint(self, known, mask, params=None, guide_w=0.0, sampler="ddpm", **sampler_kwargs):
        """Complete the maps ``known`` [n,1,H,H] where ``mask`` [n or 1,1,H,H] is 0 -> (samples, intermediate).

        ``sampler``: "ddpm" (:meth:`sample_ddpm`), "ddim" (:meth:`sample_ddim`) or "dpmpp" (:meth:`sample_dpm`); x_T and
        random params are drawn as that method draws them, and ``sampler_kwargs`` are its keywords (steps, eta, order,
        spacing, save_rate, known_noise; for "ddim" and "dpmpp" also resample, jump, t_start: with any of those "ddpm"
        raises ValueError)."""
        fns = {"ddpm": self.sample_ddpm, "ddim": self.sample_ddim, "dpmpp": self.sample_dpm}
        if sampler not in fns:
            raise ValueError(f"sampler must be 'ddpm', 'ddim' or 'dpmpp', got {sampler!r}")
        self._no_program_on_ddpm(sampler, sampler_kwargs)
        if known is None or mask is None:
            raise ValueError("masked sampling needs both known and mask")
        known = torch.as_tensor(known)
        if known.dim() != 4:
            raise ValueError(f"known must have shape [n, 1, H, H], got {tuple(known.shape)}")
        return fns[sampler](known.shape[0], self.model.h, None, params, guide_w, known=known, mask=mask,
                            **sampler_kwargs)

    @staticmethod
    def _no_program_on_ddpm(sampler, kw):
        if sampler == "ddpm" and any(k in kw for k in ("resample", "jump", "t_start")):
            raise ValueError('sampler="ddpm" takes no resample, jump or t_start: the ancestral sampler has no position '
                             'program; use sampler="ddim", eta=1.0 (its update on the timesteps you choose)')

    @torch.no_grad()
    def refine(self, init, t_start, params=None, guide_w=0.0, sampler="ddim", noise=None, known=None, mask=None,
               **sampler_kwargs):
        """Late start (SDEdit): noise the maps ``init`` [n,1,H,H] to the level t0, the largest timestep of the run that is
        <= ``t_start``, and denoise from there -> (samples, intermediate).  A small t_start re-draws only the small scales
        of ``init``; with ``known`` / ``mask`` the run also inpaints, staying close to ``init`` where it generates.

        The start state is sab[t0] init + somab[t0] noise with :func:`known_tables`' fp32 tables (the sampler's noise
        convention), two products and one sum in fp32 on the device; ``noise`` [n,1,H,H] is drawn from the CPU RNG when
        None, as the sample_* methods draw x_T.  ``sampler``: "ddim" (:meth:`sample_ddim_from_noise`) or "dpmpp"
        (:meth:`sample_dpm_from_noise`), with ``sampler_kwargs`` its keywords (steps, eta or order, spacing, save_rate,
        known_noise, resample, jump).  ValueError: "ddpm" (no position program) or an unknown sampler, ``init`` not
        [n,1,H,H], ``noise`` of another shape, and what the method raises, all before anything is drawn."""
        fns = {"ddim": (self.sample_ddim_from_noise, 50), "dpmpp": (self.sample_dpm_from_noise, 20)}
        self._no_program_on_ddpm(sampler, {"t_start": t_start})
        if sampler not in fns:
            raise ValueError(f"sampler must be 'ddim' or 'dpmpp', got {sampler!r}")
        fn, steps = fns[sampler]
        H = self.model.h
        init = torch.as_tensor(init)
        if tuple(init.shape[1:]) != (1, H, H) or init.dim() != 4:
            raise ValueError(f"init must have shape [n, 1, {H}, {H}], got {tuple(init.shape)}")
        if noise is not None and tuple(torch.as_tensor(noise).shape) != tuple(init.shape):
            raise ValueError(f"noise must have the shape of init, {tuple(init.shape)}")
        taus = timestep_subsequence(self.T, sampler_kwargs.get("steps", steps), sampler_kwargs.get("spacing", "uniform"))
        t0 = int(resample_program(self.sched.ab_t, taus, t_start=t_start).from_t[-1])
        check_inpaint(known, mask, init.shape[0], H, sampler_kwargs.get("known_noise", "fixed"), self.model.in_channels)
        if noise is None:
            noise = torch.randn(init.shape)
        sab, somab = (torch.from_numpy(v) for v in known_tables(self.sched.ab_t))
        dev = self.sched.ab_t.device
        a, b = sab[t0].to(dev), somab[t0].to(dev)
        x = a * init.to(dev, torch.float32) + b * torch.as_tensor(noise).to(dev, torch.float32)
        return fn(x, params, guide_w=guide_w, known=known, mask=mask, t_start=t_start, **sampler_kwargs)

    @torch.no_grad()
    def reconstruct(self, obs, params=None, guide_w=0.0, factor=4, weight=None, zeta=1.0, steps=50, eta=0.0,
                    spacing="uniform", noise=None, save_rate=20, z_source=None, **unsupported):
        """Draw full-resolution maps consistent with the coarse, noisy observation ``obs`` [n,1,H/factor,H/factor] (and
        with ``params``, under CFG when ``guide_w`` > 0) -> (x [n,1,H,H], intermediates, misfit [S + 1, n] fp64).

        :class:`GuidedDDIMSampler` has the definition: y = A x0 + n with A the ``factor`` x ``factor`` block mean and
        ``weight`` [n or 1,1,h,h] the relative inverse variance of every cell (0 = not observed, the way to mask; None =
        all ones); after every DDIM step of the ``steps`` positions (``eta``, ``spacing`` as :meth:`sample_ddim`) the
        state takes a step of length ``zeta`` down the gradient of the misfit norm.  misfit[S - p] = sqrt(L) seen at
        position p, the last row that of the returned x itself.  ``noise`` [n,1,H,H] fixes x_T (drawn from the CPU RNG
        when None); ``params`` None runs without context.  ``z_source`` None: this object's.  Costs, per position, one
        frozen forward and one full backward of B rows (B = 2 n with CFG) against the plain sampler's eval forward, and
        the frozen workspace's fp32 activations of B rows.  Samplers are cached per configuration, as :meth:`_sampler`
        does; the contents of obs / weight are not part of the key.  ValueError, before anything is drawn or allocated:
        what :func:`check_observation` lists, and any of sampler= (other than "ddim"), resample / jump / t_start,
        known / mask: guided sampling is the plain DDIM walk, and a zero weight is how a pixel is left unobserved."""
        if unsupported.pop("sampler", "ddim") != "ddim":
            raise ValueError('observation-guided sampling is sampler="ddim" only: "ddpm" is its eta=1.0 on all T steps, '
                             'and the multistep "dpmpp" history does not survive the guidance step')
        for k in ("resample", "jump", "t_start", "known", "mask"):
            if k in unsupported:
                raise ValueError(f"observation-guided sampling takes no {k}=: it runs the plain walk, and weight = 0 "
                                 "marks an unobserved cell")
        if unsupported:
            raise TypeError(f"reconstruct() got unexpected keyword arguments {sorted(unsupported)}")
        H = self.model.h
        obs_t = torch.as_tensor(obs) if obs is not None else None
        if obs_t is None or obs_t.dim() not in (3, 4):
            raise ValueError("obs must have shape [n, 1, H / factor, H / factor]")
        n = obs_t.shape[0]
        obs_t, wgt = check_observation(obs_t, weight, n, H, factor, zeta, self.model.in_channels)
        if noise is not None and tuple(torch.as_tensor(noise).shape) != (n, 1, H, H):
            raise ValueError(f"noise must have shape {(n, 1, H, H)}, got {tuple(torch.as_tensor(noise).shape)}")
        zs = self.z_source if z_source is None else z_source
        if zs not in ("device", "host"):
            raise ValueError(f'z_source must be "device" or "host", got {zs!r}')
        taus = timestep_subsequence(self.T, steps, spacing)
        ddim_tables(self.sched.ab_t, taus, eta)
        x_T = torch.randn(n, 1, H, H) if noise is None else torch.as_tensor(noise)
        key = ("guided", n, float(guide_w) if params is not None else 0.0, params is not None, save_rate, zs, steps,
               float(eta), spacing if isinstance(spacing, str) else tuple(spacing), int(factor), int(wgt.shape[0]),
               float(zeta))
        smp = self._samplers.get(key)
        if smp is None:
            smp = self._samplers[key] = GuidedDDIMSampler(self.model, self.sched, n, guide_w, params, steps, eta, spacing,
                                                          save_rate, zs, seed=self.seed, factor=int(factor),
                                                          weight_n=int(wgt.shape[0]), zeta=float(zeta))
        elif params is not None:
            smp.cbuf[:n] = params.to(smp.dev, torch.float32).reshape(n, -1)
        smp.prepare_rng(host_z=zs == "host")
        return smp.run(x_T, obs=obs_t, weight=wgt)

    @torch.no_grad()
    def encode(self, maps, params=None, guide_w=0.0, steps=50, spacing="uniform", save_rate=20):
        """DDIM inversion (:class:`DDIMEncoder`): the maps [n,1,H,H] (or [n,H,H]) to their latents x_T along the
        ascending walk over ``steps`` of the T timesteps (``spacing`` as :meth:`sample_ddim`) -> (x_T [n,1,H,H] on the
        device, intermediate np [slots,n,1,H,H] by ``snapshot_slots(steps, save_rate)``).  ``params`` [n, n_cfeat] or None;
        CFG when ``guide_w`` > 0.  Encoding under params c and decoding with ``sample_ddim_from_noise(x_T, c', eta=0)``
        over the same timesteps asks what the field would look like under c'.  The shortcut rows are drawn from the CPU
        RNG; nothing else is random.  Encoders are cached per configuration.  ValueError, before anything is drawn or
        allocated: maps of another shape or non-finite, params not [n, n_cfeat], a model with in_channels > 1, what
        :func:`encode_tables` raises."""
        H = self.model.h
        if self.model.in_channels != 1:
            raise ValueError("encoding is single-channel, like the samplers: the model has in_channels = "
                             f"{self.model.in_channels}")
        x, params = check_flow(maps, params, self.n_cfeat, H)
        if isinstance(guide_w, bool) or not np.isfinite(guide_w):
            raise ValueError(f"guide_w must be finite, got {guide_w!r}")
        n = x.shape[0]
        encode_tables(self.sched.ab_t, timestep_subsequence(self.T, steps, spacing))
        key = ("encode", n, float(guide_w) if params is not None else 0.0, params is not None, save_rate, steps,
               spacing if isinstance(spacing, str) else tuple(spacing))
        smp = self._samplers.get(key)
        if smp is None:
            smp = self._samplers[key] = DDIMEncoder(self.model, self.sched, n, guide_w, params, steps, spacing, save_rate,
                                                    seed=self.seed)
        elif params is not None:
            smp.cbuf[:n] = params.to(smp.dev, torch.float32).reshape(n, -1)
        smp.prepare_rng(host_z=False)
        return smp.run(x)

    @torch.no_grad()
    def log_likelihood(self, maps, params=None, steps=50, spacing="uniform", n_probe=1, form="logdet", seed=None,
                       max_rows=32, guide_w=0.0) -> FlowResult:
        """log p(x | c) of the maps [n,1,H,H] (or [n,H,H]) under ``params`` [n, n_cfeat] (None: no context) ->
        :class:`FlowResult`.  It is the log-density, per map, of the eta = 0 sampler's model at guide_w = 0, in the
        sampler's noise convention.  It is discretised at S = ``steps`` positions, with a stochastic trace estimate.  It
        is not a bound, and the reference does not compute it.  :class:`FlowLikelihood` has the walk; ``form``: "logdet"
        (default; exact where the network's Jacobian is a multiple of the identity) or "trace" (the textbook Euler step,
        first order in 1 / S).

        ``n_probe`` = R probe runs with the keys :func:`flow_run_key` (seed, r) (``seed`` None: this object's; the keys
        of different seeds do not overlap, so results may be pooled over seeds) give ``logp_probe`` [R, n], their mean
        ``logp`` and its standard error.  One sampler per chunk size serves every seed.  All maps share their probes, and the shortcut rows, drawn from the
        CPU RNG once per call, are the same for every map, probe and chunk.  The maps go in chunks of ``max_rows`` (the
        frozen workspace keeps the activations of every row of a chunk).  Cost: R * S forward + full-backward pairs per
        chunk.  ValueError, before anything is drawn or allocated: what :func:`check_flow` and :func:`encode_tables`
        list."""
        H = self.model.h
        x, params = check_flow(maps, params, self.n_cfeat, H, self.model.in_channels, guide_w, form, n_probe, max_rows)
        seed = self.seed if seed is None else seed
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 63:
            raise ValueError(f"seed must be an integer in [0, 2^63), got {seed!r}")
        taus = timestep_subsequence(self.T, steps, spacing)
        encode_tables(self.sched.ab_t, taus)
        n, D = x.shape[0], H * H
        parts, rows = [], None
        for lo in range(0, n, int(max_rows)):
            m = min(int(max_rows), n - lo)
            c = None if params is None else params[lo:lo + m]
            key = ("flow", m, params is not None, steps, spacing if isinstance(spacing, str) else tuple(spacing), form)
            smp = self._samplers.get(key)
            if smp is None:
                smp = self._samplers[key] = FlowLikelihood(self.model, self.sched, m, c, steps, spacing, form)
            elif c is not None:
                smp.cbuf[:m] = c.to(smp.dev, torch.float32).reshape(m, -1)
            if rows is None:
                smp.prepare_rng(host_z=False)
                rows = smp.sc_table.clone()
            else:
                smp.sc_table.copy_(rows)
            parts.append(smp.run(x[lo:lo + m], n_probe, seed=int(seed)))
        cat = lambda k, d: torch.cat([p[k] for p in parts], dim=d)      # noqa: E731
        logp_probe, prior, acc, hist = cat("logp", 1), cat("prior", 1), cat("acc", 1), cat("hist", 2)
        R = logp_probe.shape[0]
        logp = logp_probe.mean(0)
        stderr = logp_probe.std(0, unbiased=True) / np.sqrt(R) if R > 1 else torch.full_like(logp, float("nan"))
        logdet = (0.5 * D * parts[0]["log_abT"] + acc).mean(0)
        return FlowResult(logp, logp_probe, stderr, -logp / (D * np.log(2.0)), cat("latent", 0), prior[0], logdet, hist,
                          cat("invalid", 0), list(taus))

    def param_scan(self, maps, candidates, **kwargs):
        """:func:`cdm_amd.param_scan` of this model under this schedule: ``score[m, k]`` of every map under every
        candidate parameter vector (lower = preferred) -> ScanResult.  ``kwargs``: t_grid, n_steps, n_noise, weight, seed,
        noise, max_rows, steps_per_graph."""
        from .likelihood import param_scan
        return param_scan(self.model, maps, candidates, self.T, ab_t=self.ab_t, b_t=self.b_t, **kwargs)

    def param_fit(self, maps, start, **kwargs):
        """:func:`cdm_amd.param_fit` of this model under this schedule: gradient descent on the scan score from every
        start -> FitResult.  ``kwargs``: iters, lr, free, bounds, betas, eps, t_grid, n_steps, n_noise, weight, seed,
        noise, max_rows, steps_per_graph."""
        from .likelihood import param_fit
        return param_fit(self.model, maps, start, self.T, ab_t=self.ab_t, b_t=self.b_t, **kwargs)


@torch.no_grad()
def sample_ddpm(model, n_sample=1, size=64, device=None, params=None, guide_w=0.0, timesteps=1000, b_t=None,
                a_t=None, ab_t=None, z_source="device", *, steps=None, eta=0.0, spacing="uniform", solver="ddim",
                order=2, known=None, mask=None, known_noise="fixed"):
    """Functional sampler of code/sample_power_spectra.py:71-110 (returns the final x only).  b_t / a_t / ab_t are
    the caller's schedule, as in the reference (all three or none: None builds the default schedule).
    ``steps`` (keyword only; None: the reference's T-step ancestral sampler) runs DDPM.sample_ddim with ``eta`` and
    ``spacing`` on that many of the timesteps, or, with ``solver="dpmpp"``, DDPM.sample_dpm with ``order`` and ``spacing``
    (``solver`` is only consulted when ``steps`` is given).  ``known`` / ``mask`` / ``known_noise`` (keyword only): masked
    sampling with whichever of the three is selected, as in DDPM.sample_ddpm."""
    given = [v is not None for v in (b_t, a_t, ab_t)]
    if any(given) and not all(given):
        raise ValueError("pass all of b_t, a_t, ab_t or none of them")
    d = DDPM(model, timesteps, device or model.out[3].weight.device, z_source=z_source,
             sched_tensors=(b_t, a_t, ab_t) if all(given) else None)
    ipk = dict(known=known, mask=mask, known_noise=known_noise)
    if steps is not None:
        if solver == "dpmpp":
            return d.sample_dpm(n_sample, size, device, params, guide_w, steps, order, spacing, **ipk)[0]
        if solver != "ddim":
            raise ValueError(f"solver must be 'ddim' or 'dpmpp', got {solver!r}")
        return d.sample_ddim(n_sample, size, device, params, guide_w, steps, eta, spacing, **ipk)[0]
    return d.sample_ddpm(n_sample, size, device, params, guide_w, **ipk)[0]


def _ddpm_of(model, timesteps, device, b_t, a_t, ab_t, **kw):
    given = [v is not None for v in (b_t, a_t, ab_t)]
    if any(given) and not all(given):
        raise ValueError("pass all of b_t, a_t, ab_t or none of them")
    return DDPM(model, timesteps, device or model.out[3].weight.device,
                sched_tensors=(b_t, a_t, ab_t) if all(given) else None, **kw)


def encode(model, maps, timesteps, params=None, guide_w=0.0, b_t=None, a_t=None, ab_t=None, device=None, *, steps=50,
           spacing="uniform", save_rate=20):
    """Functional form of :meth:`DDPM.encode` on a caller's schedule, as :func:`sample_ddpm` takes one (b_t / a_t / ab_t:
    all three or none; None builds the default schedule of ``timesteps``) -> (x_T, intermediate)."""
    return _ddpm_of(model, timesteps, device, b_t, a_t, ab_t).encode(maps, params, guide_w, steps, spacing, save_rate)


def log_likelihood(model, maps, params, timesteps, b_t=None, a_t=None, ab_t=None, device=None, *, steps=50,
                   spacing="uniform", n_probe=1, form="logdet", seed=1234, max_rows=32) -> FlowResult:
    """Functional form of :meth:`DDPM.log_likelihood` on a caller's schedule (b_t / a_t / ab_t: all three or none; None
    builds the default schedule of ``timesteps``) -> :class:`FlowResult`."""
    return _ddpm_of(model, timesteps, device, b_t, a_t, ab_t).log_likelihood(maps, params, steps, spacing, n_probe, form,
                                                                            seed, max_rows)
