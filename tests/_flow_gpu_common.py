"""What the GPU tests of the flow likelihood share (test-only): the model of tests/golden/model_nf8.npz in eval mode with
randomised BatchNorm running statistics, the setting T = 100, S = 4, n = 2, bit / relative-L2 comparisons, the CPU-RNG
draws of a walk, and HIP's own ReLU / MaxPool decisions read from one frozen engine forward (tests/_kinks.py)."""
import os

import numpy as np
import torch

from oracle import ref_cpu as R
import _ddim_ref as D
from _kinks import Kinks, first_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NF, NCF, H, N, T, S = 8, 6, 64, 2, 100, 4
KW = dict(n_feat=NF, n_cfeat=NCF, height=H)


def sd():
    fx = np.load(os.path.join(GOLD, "model_nf8.npz"))
    sd = {k[3:]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith("sd.")}
    g = torch.Generator().manual_seed(11)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    return sd


_MODELS = {}


def model(math="fp32"):
    import cdm_amd
    if math not in _MODELS:
        m = cdm_amd.ContextUnet(1, NF, NCF, H, conv_math=math)
        m.load_state_dict(sd())
        _MODELS[math] = m.cuda().eval()
    return _MODELS[math]


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).cuda()


def taus():
    return D.subsequence(T, S)


def ab():
    return R.make_schedule(T)[2]


def draws(seed, eta, sets, n=N):
    """The CPU-RNG draws of one run after torch.manual_seed(seed), in the sampler's order: per position z (eta > 0 and
    p > 1), then the shortcut draw(s).  -> (rows[S - p] = [(w, b)] * sets, zs[S - p])."""
    torch.manual_seed(seed)
    rows, zs = [], []
    for p in range(S, 0, -1):
        zs.append(torch.randn(n, 1, H, H)[:, 0] if eta > 0 and p > 1 else None)
        rows.append([R.draw_shortcut(1, NF) for _ in range(sets)])
    return rows, zs


def hip_kinks_split(m, x, t, c, sc_w, sc_b, split):
    """tests/_kinks.hip_kinks for a batch whose halves take two shortcut draws (CFG: ``split`` = n < B): HIP's ReLU /
    MaxPool decisions in the oracle's call order, read from one frozen engine forward of all B rows."""
    eng, P = m._engine_and_params()
    B = x.shape[0]
    s = stream()
    eng.repack(P, True, s)
    eng.train_pack_token = object()
    m._invalidate_eval_pack()
    ws = eng.workspace(B, True, frozen=True)
    eng.forward(ws, P, x.cuda().reshape(B, H, H), t.cuda(), c.cuda(), sc_w.cuda(), sc_b.cuda(), split, s, frozen=True)
    torch.cuda.synchronize()

    def z_of(y, scale, shift, C, Sz, per_sample):
        y = y.double().cpu().reshape(B, Sz, Sz, C)
        sc_ = scale.double().cpu().reshape(B if per_sample else 1, 1, 1, C)
        sh = shift.double().cpu().reshape(B if per_sample else 1, 1, 1, C)
        return (y * sc_ + sh).float().permute(0, 3, 1, 2).contiguous()

    relu, pool = [], []
    for i, l in enumerate(eng.layers):
        st = ws.bn[l.name]
        z = z_of(ws.y[l.name], st["scale"], st["shift"], l.cout, l.S, False)
        relu.append((z > 0, z))
        if l.name in ("down1.model.1.conv2", "down2.model.1.conv2"):
            Bz, C, Sz, _ = z.shape
            r = torch.relu(z)
            win = r.reshape(Bz, C, Sz // 2, 2, Sz // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bz, C, Sz // 2, Sz // 2, 4)
            pool.append(first_max(win))
        if i == 9:
            z0 = z_of(ws.y0, ws.gn0["scale"], ws.gn0["shift"], 2 * NF, H // 4, True)
            relu.append((z0 > 0, z0))
    zO = z_of(ws.yO, ws.gnO["scale"], ws.gnO["shift"], NF, H, True)
    relu.append((zO > 0, zO))
    return relu, pool


def half(k, lo, hi):
    relu, pool = k
    return Kinks([(a[lo:hi], b[lo:hi]) for a, b in relu], [q[lo:hi] for q in pool])
