#!/usr/bin/env python3
"""Time of a graph-replayed Trainer.step() at bench.py's C2 shape (n_feat=128, bs=256, 64x64, T=1500, h3) with the
timestep-loss options off and on (loss_weight="min_snr", t_sampler="loss"): both trainers in one process on one GPU,
timed in alternating blocks of steps, a HIP event after every step.  Writes one JSON file (medians and spread).

    python tools/tloss_step_times.py --out profiles/tloss_step_times.json [--rounds 4 --steps 10 --warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NF, H, T, NCF = 128, 64, 1500, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from cdm_amd import ContextUnet, Trainer
    modes = {"default": {}, "min_snr+loss": {"loss_weight": "min_snr", "t_sampler": "loss"}}
    g = torch.Generator(device="cuda").manual_seed(1234)
    x0 = torch.rand(a.batch, 1, H, H, device="cuda", generator=g)
    c = torch.rand(a.batch, NCF, device="cuda", generator=g)
    trainers, times = {}, {k: [] for k in modes}
    for name, kw in modes.items():
        torch.manual_seed(0)
        model = ContextUnet(1, NF, NCF, H, shortcut_source="device", conv_math="h3").cuda()
        trainers[name] = Trainer(model, 1e-5, T, a.batch, seed=0, **kw)
        for _ in range(a.warmup):
            trainers[name].step(x0, c)
        assert trainers[name].graph is not None
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, tr in trainers.items():
            tr.step(x0, c)                                   # the other trainer ran last: one untimed step
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            evs[0].record()
            for k in range(a.steps):
                tr.step(x0, c)
                evs[k + 1].record()
            torch.cuda.synchronize()
            times[name].append([evs[k].elapsed_time(evs[k + 1]) for k in range(a.steps)])
    rows = []
    for name, blocks in times.items():
        flat = [v for b in blocks for v in b]
        rows.append({"mode": name, "median_ms": statistics.median(flat), "min_ms": min(flat), "max_ms": max(flat),
                     "block_medians_ms": [statistics.median(b) for b in blocks], "steps": len(flat),
                     "loss": float(trainers[name].loss.item())})
    rep = trainers["min_snr+loss"].t_loss_report()
    out = {"what": f"C2 train step (n_feat={NF}, bs={a.batch}, {H}x{H}, T={T}, h3, graph replay), one MI355X, one process, "
                   f"the two trainers timed in alternating blocks of {a.steps} steps ({a.rounds} blocks each) after "
                   f"{a.warmup} warm-up steps; hipEvent time per step",
           "rows": rows,
           "record_after": {"count_sum": int(rep["count"].sum()), "buckets_seen": int((rep["count"] > 0).sum()),
                            "prob_min": float(rep["prob"].min()), "prob_max": float(rep["prob"].max())}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
