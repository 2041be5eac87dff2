"""Canonical launch trace of the engine's forward + backward on the CPU (no GPU, no built library): per configuration
the number of library calls and a SHA-256 over every call's name and arguments.  Each non-null pointer is written as
(ordinal of its buffer by first appearance, byte offset in it, the buffer's byte size), a buffer being the merged
overlapping views of one storage, so the hash does not depend on allocator addresses or on how the workspace names
its fields: two engine versions that issue the same launches on the same operands hash the same.  The Mlp4 struct of
cdm_embed_fwd / _bwd and the job records of cdm_pack_split_conv3x3_batch are expanded the same way.

    python tools/engine_trace.py [--dump DIR]     # the table for CONFIGS (DIR: also each trace as text)
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cdm_amd._lib as LL  # noqa: E402
import cdm_amd.engine as E  # noqa: E402

# (n_feat, B, math, H, train, in_channels, frozen, attributes switched off[, also the image gradient dx])
_T = [(128, 2, "h3", 64), (128, 3, "fp32", 64), (64, 2, "h3", 64), (16, 1, "x6", 64), (128, 256, "h3", 64),
      (128, 256, "bf16", 64), (128, 1, "h3", 256), (256, 16, "h3", 256), (16, 20, "h3", 256)]
CONFIGS = ([c + (True, 1, False, ()) for c in _T]
           + [(128, 512, "h3", 64, False, 1, False, ()), (256, 32, "h3", 256, False, 1, False, ()),
              (16, 2, "h3", 64, True, 3, False, ()), (128, 2, "bf16", 64, True, 3, False, ()),
              (128, 2, "bf16", 64, True, 1, True, ()), (16, 2, "h3", 20, True, 1, False, ())]
           + [(128, 2, "h3", 64, True, 1, False, (a,)) for a in ("fuse_bn_bwd", "fuse_bn_fwd", "fuse_bn_sums",
                                                                 "batch_repack")]
           + [(128, 2, "bf16", 64, True, 1, False, (a,)) for a in ("fuse_bn_bwd", "fuse_bn_fwd", "fuse_bn_sums",
                                                                   "batch_repack", "act16")]
           + [(128, 4, "h3", 64, False, 1, False, ("fuse_eval",))]
           + [(128, 2, "h3", 64, True, 1, False, (), True), (16, 2, "h3", 64, True, 3, False, (), True)])


def eff_splits(K, s, bk=16):
    """cdm_gemm_splits on the host: the split count the library's split-K GEMMs really use."""
    kt = (K + bk - 1) // bk
    s = max(1, min(s, kt))
    per = (kt + s - 1) // s
    return (kt + per - 1) // per if kt > 0 else 1


class Recorder:
    """Stand-in for the C-ABI library: records (name, args); .extra[i] holds the pointed-to structs of call i, read at
    call time (the engine rewrites its Mlp4 between the forward and the backward)."""

    def __init__(self, protos):
        self.protos, self.calls, self.extra, self.eng = protos, [], {}, None

    def __getattr__(self, name):
        if name in self.protos:
            return lambda *a: self._call(name, a)
        if name == "raw":
            return lambda n: eff_splits if n == "cdm_gemm_splits" else (lambda *a: 0)
        raise AttributeError(name)

    def _call(self, name, a):
        if name in ("cdm_embed_fwd", "cdm_embed_bwd"):
            d = LL.Mlp4.from_address(a[0])
            self.extra[len(self.calls)] = [(f, ty is ctypes.c_void_p, getattr(m, f)) for m in d.m
                                           for f, ty in LL.MlpDesc._fields_]
        elif name == "cdm_pack_split_conv3x3_batch":
            rec = bytes(self.eng._batch_jobs.numpy())
            q = lambda o, n: int.from_bytes(rec[o:o + n], "little")  # noqa: E731
            self.extra[len(self.calls)] = [(f, n == 8, q(48 * j + o, n)) for j in range(a[1]) for f, o, n in
                                           (("W", 0, 8), ("Cin", 8, 4), ("Cout", 12, 4), ("kc", 16, 4), ("pad", 20, 4),
                                            ("wpk_x", 24, 8), ("wdg_x", 32, 8), ("amax", 40, 8))]
        self.calls.append((name, a))
        return 0


def _walk(o, out, seen):
    """Every tensor reachable from o (dicts, sequences, Acts and other __slots__ / plain objects; not the engine)."""
    if id(o) in seen or o is None or isinstance(o, (int, float, str, bool, E.UNetEngine, ctypes.Structure)):
        return
    seen.add(id(o))
    if isinstance(o, torch.Tensor):
        if o.numel():
            out.append((o.data_ptr(), o.data_ptr() + o.numel() * o.element_size()))
    elif isinstance(o, dict):
        for v in o.values():
            _walk(v, out, seen)
    elif isinstance(o, (list, tuple, set, frozenset)):
        for v in o:
            _walk(v, out, seen)
    elif type(o).__module__ == E.__name__:
        for k in list(getattr(o, "__slots__", ())) + list(getattr(o, "__dict__", {})):
            _walk(getattr(o, k, None), out, seen)


def dry_run(nf, B, math, H=64, train=True, in_channels=1, frozen=False, off=(), dx=False):
    """One forward (+ backward when train) through a recording library.  Returns (recorder, live, eng, ws): live = the
    merged [start, end) byte intervals of every tensor of the run."""
    from cdm_amd.model import ContextUnet
    rec = Recorder(LL.parse_header())
    real, E.lib = E.lib, (lambda: rec)
    try:
        eng = rec.eng = E.UNetEngine(nf, 6, H, "cpu", math, in_channels=in_channels)
        for a in off:
            assert getattr(eng, a) is True, a
            setattr(eng, a, False)
        kept = []                    # the engine's unnamed temporaries stay alive (and their addresses unique)
        buf = eng._buf
        eng._buf = lambda *a, **k: kept.append(buf(*a, **k)) or kept[-1]
        torch.manual_seed(0)
        m = ContextUnet(in_channels, nf, 6, H, conv_math=math)
        P = {k: v.detach().clone() for k, v in list(m.named_parameters()) + list(m.named_buffers())}
        eng.repack(P, train, 0)
        ws = eng.workspace(B, train, frozen) if frozen else eng.workspace(B, train)
        img = (B, H, H) if in_channels == 1 else (B * H * H, eng.cp)
        x, t, c = torch.empty(img), torch.rand(B), torch.rand(B, 6)
        sc_w, sc_b = torch.rand(2 * nf * in_channels), torch.rand(2 * nf)
        kw = {"frozen": True} if frozen else {}
        eng.forward(ws, P, x, t if train else t[:1], c, sc_w, sc_b, B if train else B // 2, 0, **kw)
        G = {n: torch.empty_like(v) for n, v in m.named_parameters()}
        deps, dx = torch.empty(img), (torch.empty(img) if dx else None)
        if train:
            eng.backward(ws, P, deps, G, 0, dx=dx)
    finally:
        E.lib = real
    iv, live = [], []
    _walk([P, G, eng.pk, ws, kept, x, t, c, sc_w, sc_b, deps, dx, eng._amax, eng._ones, eng._zeros,
           getattr(eng, "_batch_jobs", None), getattr(eng, "_batch_slots", None)], iv, set())
    for a, b in sorted(iv):
        if live and a < live[-1][1]:
            live[-1][1] = max(live[-1][1], b)
        else:
            live.append([a, b])
    return rec, [tuple(r) for r in live], eng, ws


def region(live, p):
    for a, b in live:
        if a <= p < b:
            return a, b
    return None


def canonical(rec, live):
    """(trace text, number of non-null pointers outside every live buffer)."""
    order, lines, dead = {}, [], 0

    def ptr(v):
        nonlocal dead
        if not v:
            return "null"
        r = region(live, v)
        if r is None:
            dead += 1
            return "dead"
        return f"<{order.setdefault(r, len(order))}+{v - r[0]}/{r[1] - r[0]}>"

    for i, (name, args) in enumerate(rec.calls):
        if name in ("cdm_embed_fwd", "cdm_embed_bwd"):
            args = (0,) + tuple(args[1:])           # a host struct, expanded below
        vals = [ptr(v) if ty is ctypes.c_void_p else repr(v) for v, ty in zip(args, rec.protos[name])]
        vals += [f"{f}={ptr(v) if isp else v}" for f, isp, v in rec.extra.get(i, ())]
        lines.append(name + "(" + ", ".join(vals) + ")")
    return "\n".join(lines), dead


def main():
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None   # also write each trace's text
    print("| n_feat | B | math | H | mode | in_ch | frozen | off | launches | sha256[:16] |\n" + "|---" * 10 + "|")
    for k, (nf, B, math, H, train, cin, frozen, off, *dx) in enumerate(CONFIGS):
        rec, live, _, _ = dry_run(nf, B, math, H, train, cin, frozen, off, bool(dx))
        text, dead = canonical(rec, live)
        assert dead == 0, f"{dead} pointers outside every live buffer"
        if dump:
            open(os.path.join(dump, f"{k:02d}.txt"), "w").write(text + "\n")
        print(f"| {nf} | {B} | {math} | {H} | {'train' if train else 'eval'} | {cin} | {frozen} "
              f"| {','.join(off + (('+dx',) if dx else ())) or '-'} | {len(rec.calls)} "
              f"| {hashlib.sha256(text.encode()).hexdigest()[:16]} |", flush=True)


if __name__ == "__main__":
    main()
