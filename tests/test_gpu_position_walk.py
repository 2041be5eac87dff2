"""The position walk the parameter scan and the parameter fit share (likelihood._PositionRun): a _ScanRun and a _FitRun
loaded with the same inputs leave the same bits in everything the network reads, position by position, and those bits
are the host restatement of the walk.

Shapes: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64), T = 6, M = 2, Kc = 2, t_grid = [2, 5], n_noise = 1,
table noise, use_graph=False.  No network-accuracy assertion, no Philox oracle.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NF, NCF, H, T, M, KC, T_GRID, R = 8, 6, 64, 6, 2, 2, [2, 5], 1
WALKED = ("cur_i", "cur_p", "t_cur", "sc_cur", "noise", "xt")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def model():
    import cdm_amd
    fx = np.load(os.path.join(GOLD, "model_nf8.npz"))
    m = cdm_amd.ContextUnet(1, NF, NCF, H)
    m.load_state_dict({k[3:]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith("sd.")})
    return m.cuda().eval()


def _walk(drv, run, load_c, x, pos_t, rows, z):
    """Load ``run`` and take one eager step per position -> [{name: host copy} per position], cbuf."""
    drv._refresh()
    run.load(x, load_c, pos_t, rows, z, 4321)
    run.ctr.zero_()
    s = torch.cuda.current_stream().cuda_stream
    seen = []
    for _ in range(run.npos):
        run.step(s)
        seen.append({k: getattr(run, k).cpu().clone() for k in WALKED})
    return seen, run.cbuf.cpu().clone()


def test_scan_and_fit_walk_the_same_positions(model):
    from cdm_amd.likelihood import ParamFit, ParamScan
    g = torch.Generator().manual_seed(11)
    npos = len(T_GRID) * R
    x = torch.rand(M, H, H, generator=g)
    z = torch.randn(npos, M, H, H, generator=g)
    rows = torch.randn(npos, 2 * NF, generator=g)
    cand = torch.rand(KC, NCF, generator=g)
    pos_t = torch.tensor(T_GRID * R, dtype=torch.int32)

    ps = ParamScan(model, T, use_graph=False)
    scan, scan_c = _walk(ps, ps._run(M, KC, npos, True), cand, x, pos_t, rows, z)
    pf = ParamFit(model, T, use_graph=False)
    fit, fit_c = _walk(pf, pf._run(M, KC, npos, True, R), cand[None].expand(M, -1, -1), x, pos_t, rows, z)

    assert torch.equal(scan_c, fit_c) and torch.equal(scan_c, cand.repeat(M, 1))     # row m Kc + k = candidate k
    sab, omab = ps.sched.sab.cpu(), ps.sched.omab.cpu()
    for p in range(npos):
        i = T_GRID[p % len(T_GRID)]
        want = {"cur_i": torch.tensor([i], dtype=torch.int32), "cur_p": torch.tensor([p], dtype=torch.int32),
                "t_cur": torch.tensor([i / T]),                                  # fp32 rounding of the fp64 quotient
                "sc_cur": rows[p], "noise": z[p].reshape(M, H * H),
                # two fp32 products and an fp32 sum, each rounded; every map Kc times
                "xt": (sab[i] * x + omab[i] * z[p]).repeat_interleave(KC, 0)}
        for k in WALKED:
            assert torch.equal(scan[p][k], fit[p][k]), (p, k)
            assert torch.equal(scan[p][k], want[k]), (p, k)
