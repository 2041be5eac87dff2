#!/usr/bin/env python3
"""train_diffusion.py — drop-in CLI of the reference, on the MI355X HIP engine.

    python camels-diffusion-model_amd/train_diffusion.py LR EPOCHS TIMESTEPS [NUM_PARAMS] [--options]
    torchrun --nproc-per-node N camels-diffusion-model_amd/train_diffusion.py ...      (data parallel)

Positional arguments keep the reference semantics:
  3 args  (code/train_diffusion.py:74-76)   unconditional training, n_cfeat = 5, c = None,
          outputs/BIGnoiselr_{lr}_epochs_{E}_timesteps_{T}/, checkpoints model_epoch_{ep}.pth at ep+1 in
          {25, 50, 75, 100}; afterwards the reconstruct-from-noised sampler (:163-193).
  4 args  (README.md:68-73 / code/train_diffusion_condition.py:74-77) parameter-conditioned training,
          n_cfeat = NUM_PARAMS, outputs/paper_lr_{lr}_epochs_{E}_timesteps_{T}_params_{P}/, validation MSE
          every 5 epochs, checkpoints model_epoch_{ep+1}.pth every 25 epochs and at the end; then CFG sampling
          and conditioned reconstruction of held-out maps.
Per epoch the learning rate is lr*(1 - ep/E) (:213); batch size 32, n_feat 128, 64x64 (:82-85).
Data parallel (torchrun, N ranks): --batch-size is per rank, each step is one global batch of N x batch-size
samples of the epoch's permutation split across the ranks (trainer.shard_epoch), and an epoch whose loss turned
NaN / inf stops the run (device-side counter, one read per epoch).

Data (code/train_diffusion_condition.py:104-160): Maps_HI_IllustrisTNG_LH_z=0.00.npy [N,256,256] -> shift
to positive, /max, log10, min-max to [0,1], bilinear to 64x64; params.npy [N/15, 6] repeated x15, per-column
min-max (param_min/max.npy saved), first NUM_PARAMS columns; 1500 held out with random_split(seed 42).
The CAMELS files are not in this repository (Git-LFS stubs upstream): pass --data/--params, or --synthetic N
to train on synthetic maps of the same shape.
Plots of the reference (loss curves, PDFs, P(k)) are analysis, outside the hot path: losses, samples and
timings are written as .npy / .log instead.

After the sampling (off by default; the shortcut rows of both come from the CPU RNG re-seeded with --seed):
  --encode-maps PATH.npy [--encode-params PATH.npy]
                 DDIM inversion of the maps (DDPM.encode, --loglik-steps positions) -> latents.npy
  --loglik-maps PATH.npy --loglik-params PATH.npy [--loglik-steps S --loglik-probes R --loglik-form logdet|trace]
                 the flow log-likelihood of the maps (DDPM.log_likelihood: the eta = 0 sampler's log-density, discretised
                 at S positions with R Rademacher probes; not a bound) -> log_likelihood.npz: logp, stderr, bpd, invalid, taus

Training for guided sampling (all off by default; without them the outputs are those described above):
  --p-uncond P   each sample's context is replaced by the null condition c = 0 with probability P in a step, so the
                 c = 0 forward of classifier-free guidance (--guide-w > 0) is one the model was trained on.
  --ema DECAY    keep an exponential moving average of the parameters; the sampling at the end runs on it, and every
                 model_epoch_N.pth gets a model_epoch_N_ema.pth beside it.
  --clip-grad NORM
                 clip the global L2 norm of the gradient to NORM before every Adam update (clip_grad_norm_ semantics,
                 computed on the device inside the captured step; inf: no scaling) and skip a step whose gradient holds
                 a NaN / inf; the epoch line then ends with the last gradient norm and the count of skipped steps.
  --augment none|d4|shift|d4+shift
                 train every sample of a step on a random image of itself under the symmetries of the maps: a flip and
                 quarter turns (d4), a periodic shift (shift) or both, drawn on the device inside the captured step; the
                 log gets a "Training options" line that names the mode.
  --loss-weight min_snr|PATH.npy [--snr-gamma G]   --t-sampler uniform|loss [--t-buckets NB]   --t-record
                 weight each sample's loss by its timestep (Min-SNR-gamma, G default 5, or a table of TIMESTEPS + 1
                 weights), draw the timesteps where the weighted loss is large (importance-weighted, so the objective
                 stays unbiased; single process only), or only keep the per-timestep record; any of them keeps the
                 record over min(NB, TIMESTEPS) buckets of timesteps (NB default 64) on the device inside the captured
                 step, and t_loss_record.npz (edges, count, ema_loss, prob) is written when training ends.
  --sample-steps S [--eta E] [--spacing uniform|quadratic]
                 run the sampling at the end on S of the TIMESTEPS with the strided DDIM sampler (eta 0: deterministic)
                 instead of all of them; the log lines then name steps=S, eta=E.
  --sample-steps S --sampler dpmpp [--solver-order 1|2] [--spacing ...]
                 the same S timesteps with the second-order multistep solver (DPM-Solver++ 2M, deterministic; order 1
                 is its first-order form); the log lines then name steps=S, dpmpp order=O.  Not with a non-zero --eta.
  --inpaint-known PATH.npy --inpaint-mask PATH.npy [--inpaint-noise fixed|fresh]
                 after the sampling above, complete the --n-samples maps of the first file where the mask of the second
                 is 0 (masked sampling with the sampler the flags above select; arrays [n,H,W] or [n,1,H,W], the mask
                 also [H,W]; 1 = keep the pixel) and write inpainted_samples.npy; the log gets an "Inpainting" line.
  --inpaint-resample R --inpaint-jump J
                 with the two inpaint files and --sample-steps: RePaint's resampling, each jump point of the walk
                 (every J positions) re-noised J positions back and re-denoised R - 1 times; the "Inpainting" line
                 then names resample=R, jump=J and the number of positions run.
  --refine-init PATH.npy --refine-t-start T0
                 with --sample-steps: noise the --n-samples maps of the file to the level of the largest sampled
                 timestep <= T0 and denoise from there (late start); writes refined_samples.npy and a "Refinement" line.
  --observe PATH.npy --observe-factor F [--observe-weight PATH.npy --observe-zeta Z]
                 with --sample-steps (DDIM): draw --n-samples full-resolution maps consistent with the coarse, noisy
                 observation of the file ([n,H/F,W/F] or [n,1,H/F,W/F], normalised data units; F in 1, 2, 4, 8) by
                 observation-guided sampling (cdm_amd.DDPM.reconstruct): after every DDIM step a step of length Z
                 (default 1) down the gradient of the weighted misfit norm; the weight file ([n or 1,H/F,W/F], >= 0,
                 0 = not observed) defaults to ones.  Writes reconstructed_samples.npy and reconstruct_misfit.npy
                 ([S+1,n]: the misfit norm seen at every position, then that of the written maps); the log gets an
                 "Observation-guided" line.
  --scan-maps PATH.npy --scan-candidates PATH.npy [--scan-steps S --scan-noise R --scan-weight uniform|nll]
                 conditioned runs only: after the sampling above, score every map of the first file (arrays [M,H,W] or
                 [M,1,H,W], normalised data units) under every parameter vector of the second ([K,NUM_PARAMS], normalised
                 as the training parameters are) on S of the TIMESTEPS (default min(32, TIMESTEPS)) with R noise draws
                 each, common to all candidates (cdm_amd.param_scan), and write param_scan.npz: score [M,K] (lower =
                 preferred), candidates, t_grid, best [M,NUM_PARAMS] (each map's lowest-score candidate); the log gets a
                 "Parameter scan" line.
  --fit-maps PATH.npy (--fit-start PATH.npy | --fit-from-scan K) [--fit-iters N --fit-lr LR --fit-free 0,1,...
                 --fit-steps S --fit-noise R --fit-weight uniform|nll]
                 conditioned runs only: descend the scan score of every map of the first file over the conditioning
                 parameters (cdm_amd.param_fit; Adam in fp64, clamped to [0, 1]) from the starts of the second file
                 ([NUM_PARAMS], [K,NUM_PARAMS] or [M,K,NUM_PARAMS]) or from each map's K lowest-scoring candidates of the
                 --scan-* run (which must then score the same maps); --fit-free lists the columns to fit (default all).
                 Writes param_fit.npz: params and score (the best each start visited), start, last_params,
                 history_score and history_grad_norm [N+1,M,K], t_grid, best [M,NUM_PARAMS]; the log gets a
                 "Parameter fit" line.  The score is a ranking statistic: the result is a point estimate, not a posterior.
  --resume PATH  write trainer_epoch_N.pt (parameters, BatchNorm buffers, Adam moments, EMA, step and RNG counters,
                 epoch and loss logs) beside every model checkpoint; if PATH names such a file, continue from it at
                 the epoch after the one it was written in, with that epoch's learning rate.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdm_amd.data import preprocess_maps, preprocess_params, train_test_split  # noqa: E402


def load_inpaint(known_path, mask_path, n, H):
    """The --inpaint-known / --inpaint-mask files as fp32 tensors (known [n,1,H,H], mask [n or 1,1,H,H]).  ValueError
    for a shape other than [n,H,H] / [n,1,H,H] (the mask also [H,H]) and for what cdm_amd.check_inpaint rejects."""
    from cdm_amd.diffusion import check_inpaint
    known, mask = (np.load(p, allow_pickle=False) for p in (known_path, mask_path))
    if mask.ndim == 2:
        mask = mask[None]
    out = []
    for name, v in (("known", known), ("mask", mask)):
        if v.ndim == 4 and v.shape[1] == 1:
            v = v[:, 0]
        if v.ndim != 3 or v.shape[1:] != (H, H):
            raise ValueError(f"{name} has shape {v.shape}: expected [n, {H}, {H}] or [n, 1, {H}, {H}]")
        if not (np.issubdtype(v.dtype, np.floating) or np.issubdtype(v.dtype, np.integer) or v.dtype == np.bool_):
            raise ValueError(f"{name} has dtype {v.dtype}: expected numbers")
        out.append(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))[:, None])
    known, mask = out
    if known.shape[0] != n:
        raise ValueError(f"known holds {known.shape[0]} maps, --n-samples is {n}")
    return check_inpaint(known, mask, n, H)


def load_observation(obs_path, weight_path, n, H, factor, zeta):
    """The --observe / --observe-weight files as fp32 tensors (obs [n,1,h,h], weight [n or 1,1,h,h], h = H / factor;
    no weight file: ones).  ValueError for what cdm_amd.check_observation rejects."""
    from cdm_amd.diffusion import check_observation
    obs = np.load(obs_path, allow_pickle=False)
    wgt = None if weight_path is None else np.load(weight_path, allow_pickle=False)
    if wgt is not None and wgt.ndim == 2:
        wgt = wgt[None]
    as_t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))   # noqa: E731
    return check_observation(as_t(obs), as_t(wgt), n, H, factor, zeta)


def load_maps(path, n, H):
    """The --refine-init file as an fp32 tensor [n,1,H,H].  ValueError for another shape or non-finite values."""
    v = np.load(path, allow_pickle=False)
    if v.ndim == 4 and v.shape[1] == 1:
        v = v[:, 0]
    if v.shape != (n, H, H):
        raise ValueError(f"the file has shape {v.shape}: expected [{n}, {H}, {H}] or [{n}, 1, {H}, {H}]")
    if not np.issubdtype(v.dtype, np.floating) or not np.isfinite(v).all():
        raise ValueError("the maps must be finite floating-point numbers")
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))[:, None]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lr", type=float)
    ap.add_argument("epochs", type=int)
    ap.add_argument("timesteps", type=int)
    ap.add_argument("num_params", type=int, nargs="?", default=None)
    ap.add_argument("--data", default="../data/Maps_HI_IllustrisTNG_LH_z=0.00.npy")
    ap.add_argument("--params", default="../data/params.npy")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic maps (no CAMELS files needed)")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--n-feat", type=int, default=128)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--out-root", default="outputs")
    ap.add_argument("--n-samples", type=int, default=10)
    ap.add_argument("--guide-w", type=float, default=0.0)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--p-uncond", type=float, default=0.0, help="context dropout probability (train the c = 0 branch)")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY", help="keep and sample from EMA weights")
    ap.add_argument("--clip-grad", type=float, default=None, metavar="NORM",
                    help="clip the gradient's global L2 norm to NORM; skip steps with a non-finite gradient")
    ap.add_argument("--augment", choices=["none", "d4", "shift", "d4+shift"], default="none",
                    help="symmetry augmentation inside the step: flips / quarter turns, periodic shifts, or both")
    ap.add_argument("--loss-weight", default=None, metavar="min_snr|PATH.npy",
                    help="per-timestep loss weight: Min-SNR-gamma, or a table of TIMESTEPS + 1 weights >= 0")
    ap.add_argument("--snr-gamma", type=float, default=5.0, metavar="G", help="gamma of --loss-weight min_snr")
    ap.add_argument("--t-sampler", choices=["uniform", "loss"], default="uniform",
                    help="how a step draws its timesteps: uniformly, or where the weighted loss is large")
    ap.add_argument("--t-buckets", type=int, default=64, metavar="NB", help="timestep buckets of the record (1..1024)")
    ap.add_argument("--t-record", action="store_true", help="keep the per-timestep loss record (t_loss_record.npz)")
    ap.add_argument("--resume", default=None, metavar="PATH",
                    help="write trainer_epoch_N.pt checkpoints; continue from PATH if it exists")
    ap.add_argument("--sample-steps", type=int, default=0, metavar="S",
                    help="sample on S of the TIMESTEPS (strided DDIM sampler); 0: the reference's ancestral sampler")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0 deterministic, 1 ancestral variance)")
    ap.add_argument("--spacing", choices=["uniform", "quadratic"], default="uniform",
                    help="how --sample-steps picks its timesteps")
    ap.add_argument("--sampler", choices=["ddim", "dpmpp"], default="ddim",
                    help="the update --sample-steps uses: strided DDIM, or the multistep DPM-Solver++ (2M)")
    ap.add_argument("--solver-order", type=int, choices=[1, 2], default=2, help="order of --sampler dpmpp")
    ap.add_argument("--inpaint-known", default=None, metavar="PATH.npy",
                    help="maps [n,H,W] or [n,1,H,W] (normalised data units) whose masked pixels are kept; n = --n-samples")
    ap.add_argument("--inpaint-mask", default=None, metavar="PATH.npy",
                    help="mask [n,H,W], [n,1,H,W] or [H,W] in [0, 1]: 1 = keep the pixel of --inpaint-known, 0 = generate")
    ap.add_argument("--inpaint-noise", choices=["fixed", "fresh"], default="fixed",
                    help="known-region noise: one draw for the run, or one per step")
    ap.add_argument("--inpaint-resample", type=int, default=1, metavar="R",
                    help="RePaint resampling: visit every jump point R times (needs the inpaint files and --sample-steps)")
    ap.add_argument("--inpaint-jump", type=int, default=1, metavar="J", help="jump length of --inpaint-resample, in positions")
    ap.add_argument("--refine-init", default=None, metavar="PATH.npy",
                    help="maps [n,H,W] or [n,1,H,W] (normalised data units) to re-draw from --refine-t-start; n = --n-samples")
    ap.add_argument("--refine-t-start", type=int, default=None, metavar="T0",
                    help="the timestep --refine-init is noised to (the largest sampled timestep <= T0)")
    ap.add_argument("--observe", default=None, metavar="PATH.npy",
                    help="coarse observation [n,H/F,W/F] or [n,1,H/F,W/F] (normalised data units); n = --n-samples")
    ap.add_argument("--observe-factor", type=int, default=None, metavar="F", help="block size of --observe: 1, 2, 4 or 8")
    ap.add_argument("--observe-weight", default=None, metavar="PATH.npy",
                    help="per-cell weight [n,H/F,W/F], [n,1,H/F,W/F] or [H/F,W/F], >= 0: relative inverse variance, 0 = not "
                         "observed (default: ones)")
    ap.add_argument("--observe-zeta", type=float, default=1.0, metavar="Z", help="guidance step length of --observe")
    ap.add_argument("--scan-maps", default=None, metavar="PATH.npy",
                    help="maps [M,H,W] or [M,1,H,W] (normalised data units) to score under --scan-candidates")
    ap.add_argument("--scan-candidates", default=None, metavar="PATH.npy",
                    help="candidate parameter vectors [K,NUM_PARAMS] (normalised as the training parameters)")
    ap.add_argument("--scan-steps", type=int, default=None, metavar="S",
                    help="timesteps the scan visits (default min(32, TIMESTEPS))")
    ap.add_argument("--scan-noise", type=int, default=1, metavar="R", help="noise draws per scanned timestep")
    ap.add_argument("--scan-weight", choices=["uniform", "nll"], default="uniform",
                    help="per-timestep weight of the scan's squared error: 1, or 1 / (2 b_t)")
    ap.add_argument("--fit-maps", default=None, metavar="PATH.npy",
                    help="maps [M,H,W] or [M,1,H,W] (normalised data units) whose parameters are fitted")
    ap.add_argument("--fit-start", default=None, metavar="PATH.npy",
                    help="starts [NUM_PARAMS], [K,NUM_PARAMS] or [M,K,NUM_PARAMS] (normalised as the training parameters)")
    ap.add_argument("--fit-from-scan", type=int, default=None, metavar="K",
                    help="start from each map's K lowest-scoring --scan-candidates (needs --scan-maps = the fitted maps)")
    ap.add_argument("--fit-iters", type=int, default=50, metavar="N", help="Adam steps of the fit")
    ap.add_argument("--fit-lr", type=float, default=0.02, metavar="LR", help="step size of the fit")
    ap.add_argument("--fit-free", default=None, metavar="0,1,...", help="columns to fit (default: all)")
    ap.add_argument("--fit-steps", type=int, default=None, metavar="S",
                    help="timesteps the fit visits (default min(32, TIMESTEPS))")
    ap.add_argument("--fit-noise", type=int, default=1, metavar="R", help="noise draws per fitted timestep")
    ap.add_argument("--fit-weight", choices=["uniform", "nll"], default="uniform",
                    help="per-timestep weight of the fit's squared error: 1, or 1 / (2 b_t)")
    ap.add_argument("--encode-maps", default=None, metavar="PATH.npy",
                    help="maps [n,H,W] or [n,1,H,W] (normalised data units) to encode to their DDIM latents (latents.npy)")
    ap.add_argument("--encode-params", default=None, metavar="PATH.npy",
                    help="parameters [n,NUM_PARAMS] of --encode-maps (default: no context)")
    ap.add_argument("--loglik-maps", default=None, metavar="PATH.npy",
                    help="maps [n,H,W] or [n,1,H,W] (normalised data units) whose flow log-likelihood is computed "
                         "(log_likelihood.npz)")
    ap.add_argument("--loglik-params", default=None, metavar="PATH.npy", help="parameters [n,NUM_PARAMS] of --loglik-maps")
    ap.add_argument("--loglik-steps", type=int, default=None, metavar="S",
                    help="positions of the likelihood walk, also of --encode-maps (default min(50, TIMESTEPS))")
    ap.add_argument("--loglik-probes", type=int, default=1, metavar="R", help="Rademacher probe runs")
    ap.add_argument("--loglik-form", choices=["logdet", "trace"], default="logdet",
                    help="per-step log-determinant: D log1p(g q / D), or the first-order g q")
    a = ap.parse_args(argv)
    a.flow_steps = min(50, a.timesteps) if a.loglik_steps is None else a.loglik_steps
    a.encode = a.loglik = None
    if a.encode_maps is None and a.encode_params is not None:
        ap.error("--encode-params needs --encode-maps")
    if (a.loglik_maps is None) != (a.loglik_params is None):
        ap.error("--loglik-maps and --loglik-params go together")
    for name, mp, pp in (("encode", a.encode_maps, a.encode_params), ("loglik", a.loglik_maps, a.loglik_params)):
        if mp is None:
            continue
        if a.num_params is None and pp is not None:
            ap.error(f"--{name}-params needs a conditioned run (NUM_PARAMS)")
        try:
            from cdm_amd.diffusion import check_flow, encode_tables, timestep_subsequence, Schedule
            fm = torch.from_numpy(np.load(mp, allow_pickle=False))
            fp = None if pp is None else torch.from_numpy(np.load(pp, allow_pickle=False))
            fm, fp = check_flow(fm, fp, a.num_params or 0, a.height, form=a.loglik_form, n_probe=a.loglik_probes)
            encode_tables(Schedule(a.timesteps, "cpu").ab_t, timestep_subsequence(a.timesteps, a.flow_steps, a.spacing))
            setattr(a, name, (fm.float(), None if fp is None else fp.float()))
        except (OSError, ValueError) as e:
            ap.error(f"--{name}-maps / --{name}-params: {e}")
    if (a.scan_maps is None) != (a.scan_candidates is None):
        ap.error("--scan-maps and --scan-candidates go together")
    a.scan = None
    if a.scan_maps is not None:
        if a.num_params is None:
            ap.error("--scan-maps needs a conditioned run (NUM_PARAMS)")
        try:
            from cdm_amd.likelihood import check_scan
            steps = min(32, a.timesteps) if a.scan_steps is None else a.scan_steps
            smaps, scand = (np.load(p, allow_pickle=False) for p in (a.scan_maps, a.scan_candidates))
            x, c, tg, _ = check_scan(smaps, scand, a.timesteps, a.num_params, a.height, None, steps, a.scan_noise,
                                     a.scan_weight)
            a.scan = (x, c, tg)
        except (OSError, ValueError) as e:
            ap.error(f"--scan-maps / --scan-candidates: {e}")
    a.fit = None
    if a.fit_maps is None and (a.fit_start is not None or a.fit_from_scan is not None):
        ap.error("--fit-start / --fit-from-scan need --fit-maps")
    if a.fit_maps is not None:
        if a.num_params is None:
            ap.error("--fit-maps needs a conditioned run (NUM_PARAMS)")
        if (a.fit_start is None) == (a.fit_from_scan is None):
            ap.error("--fit-maps needs exactly one of --fit-start and --fit-from-scan")
        if a.fit_from_scan is not None and a.scan is None:
            ap.error("--fit-from-scan needs --scan-maps and --scan-candidates")
        try:
            from cdm_amd.likelihood import check_fit
            free = None if a.fit_free is None else [int(v) for v in a.fit_free.split(",")]
            steps = min(32, a.timesteps) if a.fit_steps is None else a.fit_steps
            fmaps = np.load(a.fit_maps, allow_pickle=False)
            if a.fit_from_scan is not None:
                K = a.fit_from_scan
                if not 1 <= K <= a.scan[1].shape[0]:
                    raise ValueError(f"--fit-from-scan {K}: the scan has {a.scan[1].shape[0]} candidates")
                if tuple(np.squeeze(fmaps).shape) != tuple(np.squeeze(a.scan[0].numpy()).shape) or \
                        not np.array_equal(np.squeeze(fmaps).astype(np.float32), np.squeeze(a.scan[0].numpy())):
                    raise ValueError("--fit-from-scan: --fit-maps and --scan-maps must hold the same maps")
                fstart = a.scan[1][:K]                 # stands in for the scan's top K while the arguments are checked
            else:
                fstart = np.load(a.fit_start, allow_pickle=False)
            x, st, tg, _, _, _, _ = check_fit(fmaps, fstart, a.timesteps, a.num_params, a.height, a.fit_iters, a.fit_lr,
                                              free, (0.0, 1.0), (0.9, 0.999), 1e-8, None, steps, a.fit_noise,
                                              a.fit_weight)
            a.fit = (x, None if a.fit_from_scan is not None else st, tg, free)
        except (OSError, ValueError) as e:
            ap.error(f"--fit-maps / --fit-start / --fit-from-scan: {e}")
    if (a.inpaint_known is None) != (a.inpaint_mask is None):
        ap.error("--inpaint-known and --inpaint-mask go together")
    a.inpaint = None
    if a.inpaint_known is not None:
        try:
            a.inpaint = load_inpaint(a.inpaint_known, a.inpaint_mask, a.n_samples, a.height)
        except (OSError, ValueError) as e:
            ap.error(f"--inpaint-known / --inpaint-mask: {e}")
    if (a.inpaint_resample != 1 or a.inpaint_jump != 1) and (a.inpaint is None or a.sample_steps == 0):
        ap.error("--inpaint-resample / --inpaint-jump need --inpaint-known, --inpaint-mask and --sample-steps S")
    if a.inpaint_resample < 1 or a.inpaint_jump < 1:
        ap.error("--inpaint-resample and --inpaint-jump must be >= 1")
    a.observation = None
    if a.observe is None and (a.observe_factor is not None or a.observe_weight is not None):
        ap.error("--observe-factor / --observe-weight need --observe")
    if a.observe is not None:
        if a.observe_factor is None:
            ap.error("--observe needs --observe-factor F")
        if a.sample_steps == 0 or a.sampler != "ddim":
            ap.error("--observe needs --sample-steps S with the DDIM sampler (guided sampling is a strided DDIM walk)")
        try:
            a.observation = load_observation(a.observe, a.observe_weight, a.n_samples, a.height, a.observe_factor,
                                             a.observe_zeta)
        except (OSError, ValueError) as e:
            ap.error(f"--observe / --observe-weight: {e}")
    if (a.refine_init is None) != (a.refine_t_start is None):
        ap.error("--refine-init and --refine-t-start go together")
    a.refine = None
    if a.refine_init is not None:
        if a.sample_steps == 0:
            ap.error("--refine-init needs --sample-steps S (the ancestral sampler has no late start)")
        try:
            a.refine = load_maps(a.refine_init, a.n_samples, a.height)
        except (OSError, ValueError) as e:
            ap.error(f"--refine-init: {e}")
    if a.sample_steps < 0 or a.sample_steps > a.timesteps:
        ap.error(f"--sample-steps must lie in 0..TIMESTEPS = {a.timesteps}")
    if a.clip_grad is not None and not a.clip_grad > 0:
        ap.error("--clip-grad must be > 0 (inf: report the norm and skip non-finite steps only)")
    a.t_loss = a.loss_weight is not None or a.t_sampler == "loss" or a.t_record
    try:
        from cdm_amd.trainer import check_t_loss
        if a.loss_weight is not None and a.loss_weight != "min_snr":
            a.loss_weight = np.load(a.loss_weight, allow_pickle=False)
        check_t_loss(a.loss_weight if a.timesteps >= 1 else None, a.snr_gamma, a.t_sampler, a.t_buckets, 0.99, 10,
                     1e-3, max(a.timesteps, 1))
    except (OSError, ValueError) as e:
        ap.error(f"--loss-weight / --snr-gamma / --t-sampler / --t-buckets: {e}")
    if a.t_sampler == "loss" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--t-sampler loss is single process only (the ranks' timestep tables would diverge)")
    if a.sampler == "dpmpp" and a.sample_steps == 0:
        ap.error("--sampler dpmpp needs --sample-steps S")
    if a.sampler == "dpmpp" and a.eta != 0:
        ap.error("--sampler dpmpp is deterministic: it takes no --eta")

    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    import cdm_amd
    from cdm_amd import DDPM, ContextUnet, Trainer
    from cdm_amd.trainer import shard_epoch

    conditional = a.num_params is not None
    n_cfeat = a.num_params if conditional else 5
    if conditional:
        out_dir = os.path.join(a.out_root, f"paper_lr_{a.lr}_epochs_{a.epochs}_timesteps_{a.timesteps}_params_{a.num_params}")
    else:
        out_dir = os.path.join(a.out_root, f"BIGnoiselr_{a.lr}_epochs_{a.epochs}_timesteps_{a.timesteps}")
    save_dir = os.path.join(out_dir, "weights")
    if rank == 0:
        os.makedirs(save_dir, exist_ok=True)
    H = a.height

    # ------------------------------- data -------------------------------
    if a.synthetic:
        g = torch.Generator().manual_seed(1234)
        n = a.synthetic - a.synthetic % 15 if a.synthetic >= 15 else a.synthetic
        maps = torch.rand(n, 1, H, H, generator=g)
        raw_params = torch.rand(max(1, n // 15), 6, generator=g).numpy().astype(np.float64)
        params = preprocess_params(raw_params, n, n_cfeat) if n % 15 == 0 else torch.rand(n, n_cfeat, generator=g)
    else:
        torch.cuda.set_device(local)
        maps = preprocess_maps(np.load(a.data, mmap_mode="r"), H)          # device pipeline (csrc/data.hip)
        params = preprocess_params(np.load(a.params), maps.shape[0], n_cfeat, out_dir if rank == 0 else None) \
            if conditional else torch.zeros(maps.shape[0], n_cfeat)
    n_total = maps.shape[0]
    if conditional:
        # random_split(full, [n - 1500, 1500], seed 42) (:150-156); small synthetic sets hold out 10 %
        train_idx, test_idx = train_test_split(n_total, min(1500, n_total // 10), 42)
    else:
        train_idx, test_idx = torch.arange(n_total), torch.arange(0)
    # data-parallel sharding: every rank sees a disjoint slice of each epoch's permutation
    dev = torch.device("cuda", local)
    maps_d, params_d = maps.to(dev), params.to(dev)
    if rank == 0:
        with open(os.path.join(out_dir, "dataset_info.txt"), "w") as f:
            f.write(f"Total dataset size: {n_total}\nTrain dataset size: {len(train_idx)}\n"
                    f"Test dataset size: {len(test_idx)}\nNumber of parameters used for conditioning: {n_cfeat}\n"
                    f"World size: {world}\n")

    # ------------------------------- model / trainer -------------------------------
    torch.manual_seed(a.seed)
    model = ContextUnet(1, a.n_feat, n_cfeat, H).to(dev)
    trainer = Trainer(model, a.lr, a.timesteps, a.batch_size, seed=a.seed, ema_decay=a.ema, p_uncond=a.p_uncond,
                      clip_grad_norm=a.clip_grad, augment=a.augment, loss_weight=a.loss_weight, snr_gamma=a.snr_gamma,
                      t_sampler=a.t_sampler, t_record=a.t_record, t_buckets=a.t_buckets)
    log = open(os.path.join(out_dir, "timing_and_performance.log"), "a") if rank == 0 else None
    if rank == 0 and a.augment != "none":      # without the option the log is what it was
        msg = f"Training options: p_uncond={a.p_uncond:g}, ema={a.ema}, clip_grad={a.clip_grad}, augment={a.augment}"
        print(msg, flush=True)
        log.write(msg + "\n")
    loss_log, val_log = [], []
    first_ep = 0
    if a.resume is not None:
        if os.path.isfile(a.resume):
            ck = torch.load(a.resume, map_location="cpu", weights_only=True)
            trainer.load_state_dict(ck["trainer"])
            first_ep, loss_log, val_log = int(ck["epoch"]), list(ck["loss_log"]), list(ck["val_log"])
            msg = f"Resumed from {a.resume}: epoch {first_ep} done, {trainer.steps} steps"
        else:
            msg = f"No checkpoint at {a.resume}: starting at epoch 1"
        if rank == 0:
            print(msg, flush=True)
            log.write(msg + "\n")
    t_train0 = time.time()
    for ep in range(first_ep, a.epochs):
        t_ep = time.time()
        lr = a.lr * (1 - ep / a.epochs)
        trainer.set_lr(lr)
        model.train()
        order = train_idx[torch.randperm(len(train_idx), generator=torch.Generator().manual_seed(a.seed * 7919 + ep))]
        ep_loss, nb = torch.zeros(1, device=dev), 0
        # every rank runs the same number of steps; ragged global batches are weighted by sample count
        for idx, count in shard_epoch(order, a.batch_size, world, rank):
            idx = idx.to(dev)
            loss = trainer.step(maps_d[idx], params_d[idx] if conditional else None,
                                global_count=count if world > 1 and count != a.batch_size * world else None)
            ep_loss += loss
            nb += 1
        bad = trainer.check_finite()                 # SURVEY §5 failure guard: one host read per epoch
        if bad:
            raise FloatingPointError(f"epoch {ep + 1}: {bad} training step(s) produced a NaN / inf loss "
                                     f"(lr {lr:.3e}); stopping before the checkpoint is overwritten")
        torch.cuda.synchronize()
        ep_time = time.time() - t_ep
        loss_log.append(float(ep_loss.item()) / max(nb, 1))
        msg = f"Epoch {ep + 1}/{a.epochs}, Train Loss: {loss_log[-1]:.6f}, lr {lr:.3e}, epoch time {ep_time:.2f}s"
        if a.clip_grad is not None:                  # read where check_finite was read: still one sync point per epoch
            msg += f", grad norm {float(trainer.grad_norm.item()):.4e}, skipped steps {trainer.check_skipped()}"
        if conditional and (ep % 5 == 0 or ep == a.epochs - 1) and len(test_idx):
            val_log.append(validation_mse(model, maps_d[test_idx.to(dev)], params_d[test_idx.to(dev)], trainer.sched,
                                          a.timesteps, a.batch_size))
            msg += f", Val Loss: {val_log[-1]:.6f}"
        if rank == 0:
            print(msg, flush=True)
            log.write(msg + "\n"); log.flush()
            save_now = ((ep + 1) % 25 == 0 or ep == a.epochs - 1) if conditional else (ep + 1) in (25, 50, 75, 100)
            if save_now:
                name = f"model_epoch_{ep + 1}.pth" if conditional else f"model_epoch_{ep}.pth"
                torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(save_dir, name))
                n_ep = name[len("model_epoch_"):-len(".pth")]
                if a.ema is not None:
                    torch.save({k: v.cpu() for k, v in trainer.ema_state_dict().items()},
                               os.path.join(save_dir, f"model_epoch_{n_ep}_ema.pth"))
                if a.resume is not None:
                    torch.save({"trainer": trainer.state_dict(), "epoch": ep + 1, "loss_log": loss_log,
                                "val_log": val_log}, os.path.join(save_dir, f"trainer_epoch_{n_ep}.pt"))
    total_train = time.time() - t_train0
    if rank == 0:
        np.save(os.path.join(out_dir, "loss_log.npy"), np.array(loss_log))
        if val_log:
            np.save(os.path.join(out_dir, "val_loss_log.npy"), np.array(val_log))
        log.write(f"Total training time: {total_train:.2f} s\n")
        if a.t_loss:                                 # the per-timestep record (rank 0's under data parallel)
            np.savez(os.path.join(out_dir, "t_loss_record.npz"), **trainer.t_loss_report())

    # ------------------------------- sampling -------------------------------
    if not a.no_sample and rank == 0:
        # --ema: sample from the averaged weights; the live ones return afterwards
        with trainer.ema_weights() if a.ema is not None else contextlib.nullcontext():
            sample_and_compare(a, model, maps_d, params_d, test_idx, n_total, conditional, dev, H, out_dir, log)
    if log:
        log.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out_dir


def sample_and_compare(a, model, maps_d, params_d, test_idx, n_total, conditional, dev, H, out_dir, log):
    """The reference's post-training sampling (code/train_diffusion.py:163-193, train_diffusion_condition.py:301-333)."""
    import cdm_amd
    from cdm_amd import DDPM
    model.eval()
    d = DDPM(model, a.timesteps, dev)
    ns = a.n_samples
    src = test_idx if len(test_idx) else torch.arange(min(ns, n_total))
    sel = src[:ns].to(dev)
    x = maps_d[sel]
    p = params_d[sel] if conditional else None
    noise = torch.randn(x.shape, device=dev)
    x_T = cdm_amd.perturb_input(x, a.timesteps, noise, d.sched)
    t0 = time.time()
    dpm = ddim = None
    if a.sample_steps > 0 and a.sampler == "dpmpp":
        dpm = dict(steps=a.sample_steps, order=a.solver_order, spacing=a.spacing)
    elif a.sample_steps > 0:
        ddim = dict(steps=a.sample_steps, eta=a.eta, spacing=a.spacing)
    how = f"T={a.timesteps}" + (f", steps={a.sample_steps}, eta={a.eta:g}" if ddim else "") \
        + (f", steps={a.sample_steps}, dpmpp order={a.solver_order}" if dpm else "")
    if dpm:
        rec, inter = d.sample_dpm_from_noise(x_T, p, guide_w=a.guide_w, **dpm)
    elif ddim:
        rec, inter = d.sample_ddim_from_noise(x_T, p, guide_w=a.guide_w, **ddim)
    else:
        rec, inter = d.sample_ddpm_from_noise(x_T, p, guide_w=a.guide_w)
    torch.cuda.synchronize()
    dt = time.time() - t0
    np.save(os.path.join(out_dir, "reconstructed_images.npy"), rec.cpu().numpy())
    np.save(os.path.join(out_dir, "intermediate.npy"), inter)
    log.write(f"Reconstruction of {ns} maps, {how}: {dt:.2f} s\n")
    # the reference's post-sampling statistics (code/train_diffusion.py:250, diffusion_utilities.py:370),
    # on the HIP statistics kernels; the plotted arrays go to .npz files
    cdm_amd.compare_distributions(x[:, 0].cpu().numpy(), rec[:, 0].cpu().numpy(), out_dir)
    cdm_amd.compare_power_spectra(x, rec, out_dir)
    if conditional:
        t0 = time.time()
        if dpm:
            samples, _ = d.sample_dpm(ns, H, dev, p, a.guide_w, **dpm)
        elif ddim:
            samples, _ = d.sample_ddim(ns, H, dev, p, a.guide_w, **ddim)
        else:
            samples, _ = d.sample_ddpm(ns, H, dev, p, a.guide_w)
        torch.cuda.synchronize()
        dt = time.time() - t0
        np.save(os.path.join(out_dir, "generated_samples.npy"), samples.cpu().numpy())
        log.write(f"Sampling {ns} maps (w={a.guide_w}), {how}: {dt:.2f} s ({ns / dt:.3f} img/s)\n")
    if a.inpaint is not None:
        known, mask = a.inpaint
        ipk = dict(known=known, mask=mask, known_noise=a.inpaint_noise)
        rs = ""
        if (a.inpaint_resample, a.inpaint_jump) != (1, 1):
            ipk.update(resample=a.inpaint_resample, jump=a.inpaint_jump)
            taus = cdm_amd.timestep_subsequence(a.timesteps, a.sample_steps, a.spacing)
            npos = cdm_amd.resample_program(d.sched.ab_t, taus, a.inpaint_jump, a.inpaint_resample).P
            rs = f", resample={a.inpaint_resample}, jump={a.inpaint_jump}, {npos} positions"
        x_T = torch.randn(ns, 1, H, H)                       # CPU RNG, as the sample_* methods draw it
        t0 = time.time()
        if dpm:
            filled, _ = d.sample_dpm_from_noise(x_T, p, guide_w=a.guide_w, **dpm, **ipk)
        elif ddim:
            filled, _ = d.sample_ddim_from_noise(x_T, p, guide_w=a.guide_w, **ddim, **ipk)
        else:
            filled, _ = d.sample_ddpm_from_noise(x_T, p, guide_w=a.guide_w, **ipk)
        torch.cuda.synchronize()
        dt = time.time() - t0
        np.save(os.path.join(out_dir, "inpainted_samples.npy"), filled.cpu().numpy())
        log.write(f"Inpainting {ns} maps (w={a.guide_w}, {float(mask.mean()):.3f} of the pixels known, "
                  f"{a.inpaint_noise} noise{rs}), {how}: {dt:.2f} s\n")
    if a.refine is not None:
        t0 = time.time()
        kw = dict(dpm) if dpm else dict(ddim)
        refined, _ = d.refine(a.refine, a.refine_t_start, p, a.guide_w, sampler="dpmpp" if dpm else "ddim", **kw)
        torch.cuda.synchronize()
        dt = time.time() - t0
        np.save(os.path.join(out_dir, "refined_samples.npy"), refined.cpu().numpy())
        log.write(f"Refinement of {ns} maps from t_start={a.refine_t_start} (w={a.guide_w}), {how}: {dt:.2f} s\n")
    if a.observation is not None:
        obs, wgt = a.observation
        t0 = time.time()
        recon, _, misfit = d.reconstruct(obs, p, a.guide_w, factor=a.observe_factor, weight=wgt, zeta=a.observe_zeta,
                                         **ddim)
        torch.cuda.synchronize()
        dt = time.time() - t0
        np.save(os.path.join(out_dir, "reconstructed_samples.npy"), recon.cpu().numpy())
        np.save(os.path.join(out_dir, "reconstruct_misfit.npy"), misfit.numpy())
        log.write(f"Observation-guided sampling of {ns} maps (w={a.guide_w}, factor={a.observe_factor}, "
                  f"zeta={a.observe_zeta:g}, {float((wgt > 0).float().mean()):.3f} of the cells observed), {how}: "
                  f"final misfit {', '.join(f'{v:.4g}' for v in misfit[-1].tolist())}: {dt:.2f} s\n")
    if a.scan is not None:
        smaps, scand, tg = a.scan
        t0 = time.time()
        res = d.param_scan(smaps, scand, t_grid=tg, n_noise=a.scan_noise, weight=a.scan_weight)
        score = res.score.cpu().numpy()
        dt = time.time() - t0
        np.savez(os.path.join(out_dir, "param_scan.npz"), score=score, candidates=res.candidates.numpy(),
                 t_grid=np.asarray(res.t_grid, dtype=np.int64), best=res.best().numpy())
        log.write(f"Parameter scan of {score.shape[0]} maps under {score.shape[1]} candidates, {len(tg)} timesteps x "
                  f"{a.scan_noise} noise draws, weight={a.scan_weight}: {dt:.2f} s\n")
    if a.fit is not None:
        fmaps, fstart, ftg, free = a.fit
        if fstart is None:
            fstart = res.top(a.fit_from_scan)           # [M, K, NUM_PARAMS]: each map's K lowest-scoring candidates
        t0 = time.time()
        fr = d.param_fit(fmaps, fstart, iters=a.fit_iters, lr=a.fit_lr, free=free, t_grid=ftg, n_noise=a.fit_noise,
                         weight=a.fit_weight)
        fscore = fr.score.cpu().numpy()
        dt = time.time() - t0
        np.savez(os.path.join(out_dir, "param_fit.npz"), params=fr.params.cpu().numpy(), score=fscore,
                 start=fr.start.cpu().numpy(), last_params=fr.last_params.cpu().numpy(),
                 history_score=fr.history_score.cpu().numpy(), history_grad_norm=fr.history_grad_norm.cpu().numpy(),
                 t_grid=np.asarray(fr.t_grid, dtype=np.int64), best=fr.best().cpu().numpy())
        log.write(f"Parameter fit of {fscore.shape[0]} maps from {fscore.shape[1]} starts, {a.fit_iters} iterations, "
                  f"{len(ftg)} timesteps x {a.fit_noise} noise draws, weight={a.fit_weight}: {dt:.2f} s\n")
    # the shortcut rows of the two walks below come from the CPU RNG: seeded here, so the files can be reproduced from
    # the checkpoint with DDPM.encode / DDPM.log_likelihood after torch.manual_seed(SEED)
    if a.encode is not None:
        emaps, eparams = a.encode
        torch.manual_seed(a.seed)
        latents, _ = d.encode(emaps, eparams, steps=a.flow_steps, spacing=a.spacing)
        np.save(os.path.join(out_dir, "latents.npy"), latents.cpu().numpy())
        log.write(f"DDIM encoding of {emaps.shape[0]} maps, {a.flow_steps} positions\n")
    if a.loglik is not None:
        lmaps, lparams = a.loglik
        torch.manual_seed(a.seed)
        fl = d.log_likelihood(lmaps, lparams, steps=a.flow_steps, spacing=a.spacing, n_probe=a.loglik_probes,
                              form=a.loglik_form)
        np.savez(os.path.join(out_dir, "log_likelihood.npz"), logp=fl.logp.numpy(), stderr=fl.stderr.numpy(),
                 bpd=fl.bpd.numpy(), invalid=fl.invalid.numpy(), taus=np.asarray(fl.taus, dtype=np.int64))
        log.write(f"Flow log-likelihood of {lmaps.shape[0]} maps, {a.flow_steps} positions x {a.loglik_probes} probes, "
                  f"form={a.loglik_form}: {a.loglik_probes * a.flow_steps} forward + backward pairs per chunk, "
                  f"{int(fl.invalid.sum())} invalid\n")
    with open(os.path.join(out_dir, "means.txt"), "w") as f:
        f.write(f"Processed Images Mean: {x.mean().item()}\nReconstructed Images Mean: {rec.mean().item()}\n")


@torch.no_grad()
def validation_mse(model, x, c, sched, T, bs):
    """Validation pass (code/train_diffusion_condition.py:235-251): eval mode, fresh noise / t, mean MSE."""
    import cdm_amd
    model.eval()
    tot, n = 0.0, 0
    for i in range(0, x.shape[0], bs):
        xb, cb = x[i:i + bs], c[i:i + bs]
        noise = torch.randn_like(xb)
        t = torch.randint(1, T + 1, (xb.shape[0],), device=xb.device)
        xp = cdm_amd.perturb_input(xb, t, noise, sched)
        pred = model(xp, t.float() / T, cb)
        tot += F.mse_loss(pred, noise).item()
        n += 1
    model.train()
    return tot / max(n, 1)


if __name__ == "__main__":
    main()
