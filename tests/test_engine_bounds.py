"""CPU dry run of the engine's launch sequence (no GPU): every library call of a train forward + backward is
recorded through a stand-in for the C-ABI library (tools/engine_trace.py), then checked on the host — every pointer
argument lies in a live tensor of the run, and every split-K slab / fused-BN operand range fits its buffer.  Catches
workspace sizing and wiring errors before a kernel can fault on the GPU (the out.0 weight-gradient slab was once sized
only by the 18 BN layers: fine at B=256, an overflow at B=2, n_feat=128).  Every operand-extent block counts its hits,
and the configurations that must take a path assert a count above zero: a renamed entry point cannot switch its
check off."""
import collections
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cdm_hip.h")
_spec = importlib.util.spec_from_file_location("engine_trace", os.path.join(ROOT, "tools", "engine_trace.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
_eff_splits = T.eff_splits


def _param_names():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(cdm_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [p.strip().split()[-1].lstrip("*") for p in m.group(2).split(",") if p.strip()]
    return out


def _dry_run(nf, B, math, H=64, train=True, in_channels=1, frozen=False):
    rec, live, eng, _ = T.dry_run(nf, B, math, H, train, in_channels, frozen)
    _dry_run.last_eng = eng
    return rec.calls, rec.protos, live


# The bench shapes run at full size: the workspaces are torch.empty on the host, which the kernel commits only when
# touched, so B=256 (~20 GB of address space) costs < 1 GB of RSS.  Train: C2 (n_feat=128, B=256), C5 (n_feat=256,
# 256x256, B=16); eval (sampler): the CFG batch of C2 (2 x 256 images, cond + uncond halves).  in_channels = 3 runs
# the general kernels on the padded image; frozen = the forward / backward of model.eval() under autograd; H = 20: the
# generic-kernel widths.  `must`: the extent blocks the configuration has to reach.
TRAIN_H3 = ("fwd_ex", "wgrad_ex", "dgrad_bnbwd_dy", "dy_out", "x_g", "x_sums")
TRAIN_BF16 = ("fwd_ex", "wgrad_ex", "bn_bwd_dy", "x_g", "x_sums", "bf16")
CASES = [
    (128, 2, "h3", 64, True, 1, False, TRAIN_H3), (128, 3, "fp32", 64, True, 1, False, ()),
    (64, 2, "h3", 64, True, 1, False, ()), (16, 1, "x6", 64, True, 1, False, ()),
    (128, 256, "h3", 64, True, 1, False, TRAIN_H3), (128, 256, "bf16", 64, True, 1, False, TRAIN_BF16),
    (128, 1, "h3", 256, True, 1, False, ()), (256, 16, "h3", 256, True, 1, False, ()),
    (16, 20, "h3", 256, True, 1, False, ()),
    (128, 512, "h3", 64, False, 1, False, ("fwd_fused", "fused_pool")), (256, 32, "h3", 256, False, 1, False, ()),
    (16, 2, "h3", 64, True, 3, False, ()), (128, 2, "bf16", 64, True, 3, False, TRAIN_BF16),
    (128, 2, "bf16", 64, True, 1, True, ("fwd_ex", "wgrad_ex", "bn_bwd_dy", "x_g", "x_sums")),
    (16, 2, "h3", 20, True, 1, False, ()),
]


def _case_id(c):
    return "-".join(str(v) for v in c[:5]) + ("-c%d" % c[5] if c[5] > 1 else "") + ("-frozen" if c[6] else "")


@pytest.mark.parametrize("nf,B,math,H,train,in_channels,frozen,must", CASES, ids=[_case_id(c) for c in CASES])
def test_launch_arguments_stay_in_bounds(nf, B, math, H, train, in_channels, frozen, must):
    calls, protos, live = _dry_run(nf, B, math, H, train, in_channels, frozen)
    names = _param_names()
    assert len(calls) > (100 if train else 40)
    problems = []
    hits = collections.Counter()

    def need(name, a, ptr, nbytes, what):
        r = T.region(live, ptr)
        if r is None:
            problems.append(f"{name}: {what} not in a live tensor")
        elif ptr + nbytes > r[1]:
            problems.append(f"{name}: {what} overruns its buffer by {ptr + nbytes - r[1]} bytes")

    def rows(name, a, key, npix, ld, C, esz=4):
        """an activation operand: npix rows of C elements (esz bytes each) at a row stride of ld elements"""
        need(name, a, a[key], ((npix - 1) * a[ld] + a[C]) * esz, key)

    def vecs(name, a, keys, C):
        for k in keys:
            need(name, a, a[k], a[C] * 4, k)

    for name, args in calls:
        pn = names[name]
        a = dict(zip(pn, args))
        for (pname, v), ty in zip(zip(pn, args), protos[name]):
            if ty is ctypes.c_void_p and isinstance(v, int) and v and name not in ("cdm_embed_fwd", "cdm_embed_bwd"):
                if T.region(live, v) is None:
                    problems.append(f"{name}: pointer {pname} not in a live tensor")
        if name.startswith("cdm_conv3x3_wgrad"):
            K = a["N"] * a["H"] * a["W"]
            need(name, a, a["slab"], _eff_splits(K, a["splits"]) * a["Cout"] * 9 * a["Cin"] * 4, "slab")
        elif name.startswith("cdm_convT2x2_wgrad"):
            K = a["N"] * a["H"] * a["W"]
            need(name, a, a["slab"], _eff_splits(K, a["splits"]) * a["Cin"] * 4 * a["Cout"] * 4, "slab")
        elif name == "cdm_gemm_tn_f32":
            need(name, a, a["slab"], _eff_splits(a["K"], a["splits"]) * a["M"] * a["N"] * 4, "slab")
        elif name == "cdm_gemm_f32" and _eff_splits(a["K"], a["splits"]) > 1:
            need(name, a, a["slab"], _eff_splits(a["K"], a["splits"]) * a["M"] * a["N"] * 4, "slab")
        elif name == "cdm_conv3x3_cout1_wgrad":
            nblk = a["N"] * a["H"] // -a["csize"] if a["csize"] < 0 else a["N"] * -(-a["H"] * a["W"] // a["csize"])
            need(name, a, a["slab"], nblk * 9 * a["C"] * 4, "slab")
        elif name == "cdm_slab_reduce":
            need(name, a, a["slab"], a["splits"] * a["M"] * a["N"] * 4, "slab")
        if name == "cdm_pack_split_conv3x3_batch":
            import numpy as np
            tab = _dry_run.last_eng._batch_jobs.numpy()
            assert a["jobs_dev"] == _dry_run.last_eng._batch_jobs.data_ptr() and a["njobs"] * 48 == tab.size
            for j in range(a["njobs"]):
                rec = tab[48 * j:48 * (j + 1)]
                Wp, wx, wd, am = (int(np.frombuffer(rec[o:o + 8].tobytes(), np.uint64)[0]) for o in (0, 24, 32, 40))
                cin, cout, kc = (int(np.frombuffer(rec[o:o + 4].tobytes(), np.int32)[0]) for o in (8, 12, 16))
                assert cin * cout * 9 <= a["max_w_elems"]
                need(name, a, Wp, cin * cout * 9 * 4, f"job {j} W")
                need(name, a, wx, -(-9 * cin // 16) * 3 * cout * 16 * 2, f"job {j} wpk_x")
                if wd:
                    need(name, a, wd, -(-9 * cout // 16) * 3 * cin * 16 * 2, f"job {j} wdg_x")
                need(name, a, am, 4, f"job {j} amax")
        # element sizes from the dt bits (include/cdm_hip.h): forward / dgrad: bit 0 the source, bit 1 the output;
        # weight gradient: bit 0 g / dy / y, bit 1 x / x_g
        dt = a.get("dt", 0)
        e0, e1 = (2 if dt & 1 else 4), (2 if dt & 2 else 4)
        Pn = a["N"] * a["H"] * a["W"] if {"N", "H", "W"} <= a.keys() else 0
        if dt:
            hits["bf16"] += 1
        if name in ("cdm_conv3x3_fwd_x16", "cdm_conv3x3_fwd_x16_ex"):
            rows(name, a, "x", Pn, "ldx", "Cin", e0)
            rows(name, a, "y", Pn, "ldy", "Cout", e1)
        if name == "cdm_conv3x3_fwd_x16_ex":
            hits["fwd_ex"] += 1
            if a["pre_s"]:
                vecs(name, a, ("pre_s", "pre_t"), "Cin")
            if a["ymm"]:
                need(name, a, a["ymm"], a["Cout"] * 4, "ymm max")
                need(name, a, a["ymm"] + 4 * a["ymm_ld"], a["Cout"] * 4, "ymm min")
        if name == "cdm_conv3x3_wgrad_x16_ex":
            hits["wgrad_ex"] += 1
            rows(name, a, "g", Pn, "ldg", "Cout", e0)
            if a["y"]:
                rows(name, a, "y", Pn, "ldy", "Cout", e0)
            rows(name, a, "x", Pn, "ldx", "Cin", e1)
            if a["x_s"]:
                vecs(name, a, ("x_s", "x_t"), "Cin")
            if a["x_g"]:
                hits["x_g"] += 1
                rows(name, a, "x_g", Pn, "ldxg", "Cin", e1)
            if a["x_sums"]:
                hits["x_sums"] += 1
                vecs(name, a, ("x_mean", "x_invstd"), "Cin")
                need(name, a, a["x_sums"], _eff_splits(Pn, a["splits"]) * 3 * (a["Cout"] // 128) * 5 * a["Cin"] * 4,
                     "x_sums")
        if name == "cdm_bn_fwd_finalize" and a["ymm"]:
            need(name, a, a["ymm"], a["C"] * 4, "ymm max")
            need(name, a, a["ymm"] + 4 * a["ymm_ld"], a["C"] * 4, "ymm min")
        if name == "cdm_conv3x3_dgrad_x16_bnbwd_dy":
            hits["dgrad_bnbwd_dy"] += 1
            rows(name, a, "g", Pn, "ldg", "C", e0)
            rows(name, a, "y", Pn, "ldy", "C", e0)
            vecs(name, a, ("s", "t", "mean", "invstd", "A", "B", "Cc"), "C")
            rows(name, a, "out", Pn, "ldo", "Cout", e1)
            if a["dy_out"]:
                hits["dy_out"] += 1
                rows(name, a, "dy_out", Pn, "ldg", "C", e0)
        if name == "cdm_bn_bwd_dy":
            hits["bn_bwd_dy"] += 1
            rows(name, a, "g", a["P"], "ldg", "C", e0)
            rows(name, a, "y", a["P"], "ldy", "C", e0)
            vecs(name, a, ("s", "t", "mean", "invstd", "A", "B", "Cc"), "C")
            rows(name, a, "dy", a["P"], "lddy", "C", e1)
        if name == "cdm_conv3x3_fwd_x16_fused":
            hits["fwd_fused"] += 1
            rows(name, a, "x", Pn, "ldx", "Cin")
            need(name, a, a["bias"], a["Cout"] * 4, "bias")
            if a["kind"] == 3:      # the pooled map [N][H/2][W/2]
                hits["fused_pool"] += 1
                rows(name, a, "y", a["N"] * (a["H"] // 2) * (a["W"] // 2), "ldy", "Cout")
            else:
                rows(name, a, "y", Pn, "ldy", "Cout")
            if a["kind"] == 1:
                need(name, a, a["sc_x"], Pn * 4, "sc_x")
                ndraw = 2 if a["split"] < a["N"] else 1
                need(name, a, a["sc_w"], ndraw * a["Cout"] * 4, "sc_w")
                need(name, a, a["sc_b"], ndraw * a["Cout"] * 4, "sc_b")
            if a["kind"] == 2:
                need(name, a, a["fa"], ((a["N"] - 1) * a["fan"] + a["Cout"]) * 4, "fa")
                need(name, a, a["fb"], ((a["N"] - 1) * a["fbn"] + a["Cout"]) * 4, "fb")
    assert not problems, problems[:10]
    missed = [k for k in must if not hits[k]]
    assert not missed, f"extent checks that never ran: {missed} (hits {dict(hits)})"
