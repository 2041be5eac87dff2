#!/usr/bin/env python3
"""Time one strided (DDIM) sampling run against the full T-step run at the benchmark's sampling shape.

    python tools/ddim_bench.py [--out FILE] [--n 256] [--n-feat 128] [--T 1500] [--steps 50]

For w = 0 and w = 3: GraphSampler over all T steps and DDIMSampler over --steps of them (eta = 0, uniform), each timed
with events around one run() after a warm run (the full sampler's warm run is 2 graph replays: same kernels, same
graph), device z.  Prints and optionally writes one JSON object with the total and per-step times.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-feat", type=int, default=128)
    ap.add_argument("--T", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--conv-math", default="h3")
    a = ap.parse_args()
    import cdm_amd
    from cdm_amd.diffusion import DDIMSampler, GraphSampler, Schedule
    torch.manual_seed(0)
    model = cdm_amd.ContextUnet(1, a.n_feat, 6, 64, conv_math=a.conv_math).cuda().eval()
    sched = Schedule(a.T, "cuda")
    params = torch.rand(a.n, 6, generator=torch.Generator().manual_seed(77))
    x_T = torch.randn(a.n, 1, 64, 64, generator=torch.Generator().manual_seed(99))
    res = {"n": a.n, "n_feat": a.n_feat, "T": a.T, "steps": a.steps, "conv_math": a.conv_math,
           "device": torch.cuda.get_device_name(0), "runs": []}
    for w in (0.0, 3.0):
        full = GraphSampler(model, sched, a.n, w, params, z_source="device")
        full.prepare_rng(host_z=False)
        full.run(x_T, steps=2 * full.K)
        ms_full = timed(lambda: full.run(x_T))
        del full
        torch.cuda.empty_cache()
        sub = DDIMSampler(model, sched, a.n, w, params, steps=a.steps, eta=0.0, z_source="device")
        sub.prepare_rng(host_z=False)
        sub.run(x_T)
        ms_sub = timed(lambda: sub.run(x_T))
        del sub
        torch.cuda.empty_cache()
        row = {"w": w, "full_ms": round(ms_full, 2), "full_ms_per_step": round(ms_full / a.T, 4),
               "ddim_ms": round(ms_sub, 2), "ddim_ms_per_step": round(ms_sub / a.steps, 4),
               "speedup": round(ms_full / ms_sub, 2)}
        print(row, flush=True)
        res["runs"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
