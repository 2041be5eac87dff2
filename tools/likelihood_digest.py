"""Digests of the likelihood, scan, fit and sampler outputs of one source tree, to compare two trees bit for bit.

    python tools/likelihood_digest.py --root TREE > tree.jsonl
    python tools/likelihood_digest.py --compare parent.jsonl new.jsonl --out profiles/likelihood_refactor_digest.json

Imports ``cdm_amd`` from TREE (its library must be built) and runs a fixed list of small cases on the nf8 golden model
(n_feat 8, 64x64) under both conv arithmetics, ``torch.manual_seed`` set before each.  One JSON line per case: the
SHA-256 of the raw bytes of every output tensor.  Then, in a second process with CDM_TRACE_CALLS=1 (every library call
named on stderr and synchronised), the eager cases again: one line per case with the SHA-256 of the sequence of call
names, which shows that no launch was added, dropped or reordered.  ``--compare`` joins two such files case by case.
"""
import argparse
import hashlib
import io
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(os.path.dirname(HERE), "tests", "golden", "model_nf8.npz")
NF, NCF, H = 8, 6, 64


def _sha(v):
    import numpy as np
    import torch
    if torch.is_tensor(v):
        v = v.detach().cpu().contiguous().numpy()
    return hashlib.sha256(np.ascontiguousarray(np.asarray(v)).tobytes()).hexdigest()


def _cases(cdm, model, eager_only):
    """(name, thunk -> {output name: tensor, array or float}) for every case; ``eager_only`` drops the graph ones."""
    import torch
    from cdm_amd.likelihood import LikelihoodEvaluator, ParamFit, ParamScan
    g = torch.Generator().manual_seed(2024)
    x = torch.rand(5, 1, H, H, generator=g)
    c = torch.rand(5, NCF, generator=g)
    graphs = (False,) if eager_only else (True, False)

    def nll(ns, ug):
        ev = LikelihoodEvaluator(model, 6, ns, steps_per_graph=4, use_graph=ug)     # one replay + two eager steps
        out = {}
        for name, xb, cb in (("b3", x[:3], c[:3]), ("b2_ragged", x[3:], c[3:]), ("b3_no_c", x[:3], None),
                             ("b3_again", x[:3], c[:3])):
            out[name] = ev.batch_nll(xb, cb).clone()
        return out

    def dataset(ns):
        batches = [(x[:3], c[:3]), (x[3:], c[3:])]
        elbo, bpd = cdm.calculate_elbo_and_bpd(model, batches, 12, noise_source=ns)
        return {"elbo": elbo, "bpd": bpd, "nll": cdm.calculate_likelihood(model, batches, 12, noise_source=ns)}

    maps, cand = x[:2, 0], c[:3]
    kw = dict(t_grid=[1, 3, 6], n_noise=2, max_rows=4)                # six positions; chunks of 2 and 1
    table = torch.randn(6, 2, H, H, generator=g)
    lo, hi = torch.zeros(NCF), torch.full((NCF,), 0.9)

    def scan(noise, weight, ug):
        ps = ParamScan(model, 6, steps_per_graph=4, use_graph=ug)
        return {f"seed{seed}_{n}": ps.scan(maps, cand, weight=weight, seed=seed, noise=noise, **kw).score
                for n, seed in enumerate((4321, 4321, 99))}

    def fit(noise, weight, ug):
        pf = ParamFit(model, 6, steps_per_graph=4, use_graph=ug)
        r = pf.fit(maps, cand * 0.9, iters=3, free=[0, 2], bounds=(lo, hi), weight=weight, noise=noise, **kw)
        out = {k: getattr(r, k) for k in ("params", "score", "last_params", "start", "start_score", "history_score",
                                          "history_grad_norm", "stalled")}
        out["value"], out["grad"] = pf.value_and_grad(maps, cand, weight=weight, noise=noise, **kw)
        return out

    def sample(kind, eta, ug):
        sched = cdm.Schedule(6, "cuda")
        out = {}
        for name, short in (("full", 0), ("short", 1)):
            kws = dict(z_source="host", use_graph=ug)
            if kind == "ddpm":
                smp = cdm.GraphSampler(model, sched, 2, 0.0, c[:2], steps_per_graph=4, **kws)
            elif kind == "ddim":
                smp = cdm.DDIMSampler(model, sched, 2, 0.0, c[:2], steps=3, eta=eta, steps_per_graph=2, **kws)
            else:
                smp = cdm.DPMSolverSampler(model, sched, 2, 0.0, c[:2], steps=3, steps_per_graph=2, **kws)
            x_T = torch.randn(2, 1, H, H)
            smp.prepare_rng(host_z=True)
            xs, inter = smp.run(x_T, steps=smp.npos - short)
            out[name + "_x"] = xs
            if not short:                   # a run stopped early leaves the last snapshot slot as torch.empty made it
                out[name + "_inter"] = inter
        return out

    for ug in graphs:
        tag = "graph" if ug else "eager"
        for ns in ("device", "host"):
            yield f"nll_{ns}_{tag}", lambda ns=ns, ug=ug: nll(ns, ug)
        for noise, nname in ((None, "device"), (table, "table")):
            for weight in ("uniform", "nll"):
                yield f"scan_{nname}_{weight}_{tag}", lambda a=(noise, weight, ug): scan(*a)
                yield f"fit_{nname}_{weight}_{tag}", lambda a=(noise, weight, ug): fit(*a)
        for kind, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 1.0), ("dpmpp", 0.0)):
            yield f"sample_{kind}_eta{eta:g}_{tag}", lambda a=(kind, eta, ug): sample(*a)
    if not eager_only:                                  # the drivers cached on the model: graphs, default steps per graph
        for ns in ("device", "host"):
            yield f"dataset_{ns}", lambda ns=ns: dataset(ns)


def _run(root, trace):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    import cdm_amd as cdm
    fx = np.load(GOLD)
    sd = {k[3:]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith("sd.")}
    for cm in ("fp32", "h3"):
        model = cdm.ContextUnet(1, NF, NCF, H, conv_math=cm)
        model.load_state_dict(sd)
        model = model.cuda().eval()
        for name, thunk in _cases(cdm, model, trace):
            torch.manual_seed(1234)
            line = {"case": f"{cm}/{name}"}
            if trace:
                err, sys.stderr = sys.stderr, io.StringIO()
                try:
                    thunk()
                    names = [ln.split()[1] for ln in sys.stderr.getvalue().splitlines() if ln.startswith("[cdm] ")]
                finally:
                    sys.stderr = err
                line["case"] += "/calls"
                line["digest"] = {"n_calls": len(names), "sequence": hashlib.sha256("\n".join(names).encode()).hexdigest()}
            else:
                line["digest"] = {k: _sha(v) for k, v in thunk().items() if v is not None}
            torch.cuda.synchronize()
            print(json.dumps(line), flush=True)


def _compare(a, b, out):
    load = lambda p: {r["case"]: r["digest"] for r in map(json.loads, open(p)) if "case" in r}
    A, B = load(a), load(b)
    cases = [{"case": k, "parent": A.get(k), "new": B.get(k), "equal": A.get(k) == B.get(k)} for k in sorted(set(A) | set(B))]
    res = {"parent": a, "new": b, "n_cases": len(cases), "all_equal": all(r["equal"] for r in cases), "cases": cases}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"n_cases": len(cases), "all_equal": res["all_equal"],
                      "unequal": [r["case"] for r in cases if not r["equal"]]}))
    return 0 if res["all_equal"] and cases else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", help="the source tree to import cdm_amd from")
    ap.add_argument("--trace", action="store_true", help="(the second process) hash the library call sequences")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--out", default="likelihood_digest_compare.json")
    args = ap.parse_args()
    if args.compare:
        return _compare(*args.compare, args.out)
    if not args.root:
        ap.error("--root or --compare")
    if args.trace:
        _run(args.root, True)
        return 0
    _run(args.root, False)
    env = dict(os.environ, CDM_TRACE_CALLS="1")
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.root, "--trace"], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
