"""The parts every sampler shares: the step prologue's range guard, the one host draw loop of prepare_rng (against a
straight-line restatement of the order the class docstrings document) and its error for a sampler without host tables.

Shapes: tests/golden/model_nf8.npz (n_feat 8, n_cfeat 6, 64x64), n = 2, T = 6, S = 3.  No network evaluation.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NF, NCF, H, N, T, S = 8, 6, 64, 2, 6, 3


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


def _build(model, kind, eta, inpaint, w, z_source):
    """kind: "ddpm" (GraphSampler, T positions), "ddim" or "dpmpp" (S positions)."""
    import cdm_amd
    sched = cdm_amd.Schedule(T, "cuda")
    params = torch.rand(N, NCF, generator=torch.Generator().manual_seed(3))
    kw = dict(z_source=z_source, inpaint=inpaint)
    if kind == "ddpm":
        return cdm_amd.GraphSampler(model, sched, N, w, params, **kw)
    if kind == "ddim":
        return cdm_amd.DDIMSampler(model, sched, N, w, params, steps=S, eta=eta, **kw)
    return cdm_amd.DPMSolverSampler(model, sched, N, w, params, steps=S, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. the prologue's range guard
# ---------------------------------------------------------------------------------------------------------------
def test_prologue_guard_and_in_range_values():
    """cdm_sample_prologue, T = 4, shortcut rows of 8: a counter of 0 or 5 leaves ctr, cur_i, t_cur and sc_cur at their
    sentinel bits; 4..1 write i, fp32(i / T) and row T - i.  The table has a spare row on each side of the T real ones
    (rows T - 5 = -1 and T - 0 = T of the real table), so a missing guard copies a spare row: a failure, not a read
    outside the allocation."""
    import cdm_amd
    lb = cdm_amd.lib()
    T_, row = 4, 8
    buf = torch.randn(T_ + 2, row, generator=torch.Generator().manual_seed(5))
    buf_d = buf.cuda()
    table_ptr = buf_d[1:].data_ptr()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    cur_i = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_cur = torch.zeros(1, device="cuda")
    sc_cur = torch.zeros(row, device="cuda")

    def launch():
        lb.cdm_sample_prologue(ctr.data_ptr(), T_, cur_i.data_ptr(), t_cur.data_ptr(), table_ptr, row,
                               sc_cur.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for bad in (0, T_ + 1):
        ctr.fill_(bad); cur_i.fill_(-7); t_cur.fill_(-3.5); sc_cur.fill_(-9.0)
        launch()
        assert ctr.item() == bad and cur_i.item() == -7
        assert torch.equal(t_cur.cpu(), torch.tensor([-3.5])) and torch.equal(sc_cur.cpu(), torch.full((row,), -9.0))
    ctr.fill_(T_)
    for i in range(T_, 0, -1):
        launch()
        assert ctr.item() == i - 1 and cur_i.item() == i
        assert torch.equal(t_cur.cpu(), torch.tensor([i / T_]))
        assert torch.equal(sc_cur.cpu(), buf[1 + T_ - i])
    assert torch.equal(buf_d.cpu(), buf)


# ---------------------------------------------------------------------------------------------------------------
# 2. host draw order
# ---------------------------------------------------------------------------------------------------------------
def _restated_draws(kind, eta, inpaint, sets):
    """The CPU-RNG order of a host_z run as GraphSampler, DDIMSampler and DPMSolverSampler document it -> (shortcut
    table, z rows, xi rows), consuming the global CPU generator."""
    npos = T if kind == "ddpm" else S
    rows, zs, xis = [], [], []
    if inpaint == "fixed":                                   # one xi for the run, before the loop over the positions
        xis.append(torch.randn(N, 1, H, H))
    for p in range(npos, 0, -1):
        if p > 1 and (kind == "ddpm" or (kind == "ddim" and eta > 0)):       # z; the solver of "dpmpp" draws none
            zs.append(torch.randn(N, 1, H, H))
        if inpaint == "fresh" and p > 1:                     # after that position's z, before its shortcut row(s)
            xis.append(torch.randn(N, 1, H, H))
        ws, bs = [], []
        for _ in range(sets):                                # cond before uncond
            conv = torch.nn.Conv2d(1, NF, kernel_size=1, stride=1, padding=0)
            ws.append(conv.weight.detach().reshape(NF)); bs.append(conv.bias.detach())
        rows.append(torch.cat(ws + bs))
    flat = lambda v: torch.stack(v).reshape(len(v), -1) if v else None
    return torch.stack(rows), flat(zs), flat(xis)


_DRAW_CASES = [(kind, eta, inpaint, 0.0) for kind, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 1.0), ("dpmpp", 0.0))
               for inpaint in (None, "fixed", "fresh")]
_DRAW_CASES += [("ddim", 1.0, inpaint, 3.0) for inpaint in (None, "fixed", "fresh")]       # CFG: two shortcut sets


@pytest.mark.parametrize("kind,eta,inpaint,w", _DRAW_CASES)
def test_host_draw_order(model, kind, eta, inpaint, w):
    """prepare_rng(host_z=True) fills sc_table, z_table and xi_table with exactly the restated draws and leaves the CPU
    generator where the restatement leaves it; a table nothing is drawn for does not exist."""
    smp = _build(model, kind, eta, inpaint, w, "host")
    assert smp.sets == (2 if w > 0 else 1) and smp.npos == (T if kind == "ddpm" else S)
    torch.manual_seed(77)
    smp.prepare_rng(host_z=True)
    state = torch.get_rng_state()
    torch.manual_seed(77)
    rows, zs, xis = _restated_draws(kind, eta, inpaint, smp.sets)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(smp.sc_table.cpu(), rows)
    for table, want in ((smp.z_table, zs), (smp.xi_table, xis)):
        assert (table is None) == (want is None)
        if want is not None:
            assert torch.equal(table.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------
# 3. host_z without host tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inpaint", [None, "fixed"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmpp"])
def test_host_z_needs_host_tables(model, kind, inpaint):
    smp = _build(model, kind, 1.0, inpaint, 0.0, "device")
    with pytest.raises(ValueError, match="z_source"):
        smp.prepare_rng(host_z=True)
