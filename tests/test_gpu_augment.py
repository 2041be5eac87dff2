"""Symmetry augmentation on the device (Trainer(augment=...), cdm_amd.augment_maps / draw_augment_ops).

Everything here is bit-exact: the augmentation is a gather, the perturb expression is cdm_perturb's, the draw is an
integer function of the uniforms cdm_philox_uniform writes.

  * cdm_perturb_aug with noise == NULL (augment_maps) against the torch restatement (tests/_augment_ref.py), odd H and
    H = 16, all eight g, dy != dx, dy = H - 1; with noise, against cdm_perturb on the restated maps, per-sample t; with
    all-zero ops, against cdm_perturb on the raw maps.
  * cdm_augment_draw against the formula applied to cdm_philox_uniform's output for the same seed and sub; ranges,
    coverage and the g counts at B = 4096 (512 +- 127 = 6 binomial sigmas, sqrt(4096 / 8 * 7 / 8) = 21.2); the modes.
  * Trainer: fixed ops on the raw batch == no augmentation on the restated batch; graph replay == eager with device
    draws; resume; a checkpoint of another mode raises; augment="none" is the default trainer; x0 stays intact.
"""
import pytest
import torch

from _augment_ref import augment_ref

pytestmark = pytest.mark.gpu
INVALID = 1          # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ops_covering(H):
    """Three batches of three ops: all eight g (and the identity once more), dy != dx nonzero, dy = H - 1."""
    return [torch.tensor([[0, 0, 0], [1, H - 1, 2], [2, 1, H - 2]]), torch.tensor([[3, 2, 1], [4, H - 1, 1], [5, 0, 3]]),
            torch.tensor([[6, 3, 0], [7, 1, H - 1], [0, H - 1, 2]])]


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("four_d", [False, True])
@pytest.mark.parametrize("H", [5, 16])
def test_augment_maps_equals_the_restatement(H, four_d):
    import cdm_amd
    B = 3
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, 1, H, H, generator=g) if four_d else torch.randn(B, H, H, generator=g)
    xd = x.cuda()
    seen = set()
    for ops in _ops_covering(H):
        seen.update(int(v) for v in ops[:, 0])
        out = cdm_amd.augment_maps(xd, ops.cuda())
        assert out.shape == x.shape and out.device.type == "cuda"
        assert torch.equal(_bits(out), _bits(augment_ref(x, ops))), ops.tolist()
        assert torch.equal(cdm_amd.augment_maps(xd, ops.int()).cpu(), out.cpu()), "host int32 ops"
    assert seen == set(range(8))
    assert torch.equal(xd.cpu(), x), "the input was written"
    with pytest.raises(ValueError):
        cdm_amd.augment_maps(xd, torch.tensor([[8, 0, 0], [0, 0, 0], [0, 0, 0]]))
    with pytest.raises(ValueError):
        cdm_amd.augment_maps(xd, torch.tensor([[0, H, 0], [0, 0, 0], [0, 0, 0]]))
    with pytest.raises(ValueError):
        cdm_amd.augment_maps(xd[:, ..., :-1], torch.zeros(B, 3, dtype=torch.int32))


def _perturb(L, sched, x, noise, t, T, ops=None):
    B, H = x.shape[0], x.shape[-1]
    out = torch.full_like(x, float("nan"))
    tin = torch.full((B,), float("nan"), device="cuda")
    if ops is None:
        L.cdm_perturb(x.data_ptr(), noise.data_ptr(), t.data_ptr(), None, 0, sched.sab.data_ptr(), sched.omab.data_ptr(),
                      B, H * H, T, out.data_ptr(), tin.data_ptr(), _s())
    else:
        L.cdm_perturb_aug(x.data_ptr(), ops.data_ptr(), noise.data_ptr(), t.data_ptr(), None, 0, sched.sab.data_ptr(),
                          sched.omab.data_ptr(), B, H * H, H, T, out.data_ptr(), tin.data_ptr(), _s())
    torch.cuda.synchronize()
    return out, tin


def test_perturb_aug_equals_perturb_on_the_restated_maps():
    import cdm_amd
    L = cdm_amd.lib()
    B, H, T = 3, 16, 10
    sched = cdm_amd.Schedule(T, "cuda")
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, H, H, generator=g)
    noise = torch.randn(B, H, H, generator=g).cuda()
    t = torch.tensor([1, 10, 4], dtype=torch.int32, device="cuda")
    xd = x.cuda()
    for ops in _ops_covering(H):
        got, tin = _perturb(L, sched, xd, noise, t, T, ops.int().cuda())
        want, tin_ref = _perturb(L, sched, augment_ref(x, ops).cuda(), noise, t, T)
        assert torch.equal(_bits(got), _bits(want)), ops.tolist()
        assert torch.equal(_bits(tin), _bits(tin_ref))
    zero = torch.zeros(B, 3, dtype=torch.int32, device="cuda")
    got, tin = _perturb(L, sched, xd, noise, t, T, zero)
    want, tin_ref = _perturb(L, sched, xd, noise, t, T)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(tin), _bits(tin_ref))
    assert torch.equal(xd.cpu(), x), "the input was written"


def test_entry_point_argument_checks():
    import cdm_amd
    L = cdm_amd.lib()
    B, H = 2, 4
    x = torch.ones(B, H, H, device="cuda")
    out = torch.full_like(x, 5.0)
    ops = torch.zeros(B, 3, dtype=torch.int32, device="cuda")
    raw = L.raw("cdm_perturb_aug")

    def gather(x_=x.data_ptr(), ops_=ops.data_ptr(), out_=out.data_ptr(), N=B, HW=H * H, H_=H):
        return raw(x_, ops_, None, None, None, 0, None, None, N, HW, H_, 0, out_, None, _s())
    for kw in (dict(x_=None), dict(ops_=None), dict(out_=None), dict(out_=x.data_ptr()), dict(N=0), dict(H_=0),
               dict(HW=H * H + 1)):
        assert gather(**kw) == INVALID, kw
    noise = torch.zeros_like(x)
    # with noise: neither t nor cur_i
    assert raw(x.data_ptr(), ops.data_ptr(), noise.data_ptr(), None, None, 0, x.data_ptr(), x.data_ptr(), B, H * H, H,
               10, out.data_ptr(), None, _s()) == INVALID
    draw = L.raw("cdm_augment_draw")
    filled = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    for args in ((None, B, H, 3), (filled.data_ptr(), 0, H, 3), (filled.data_ptr(), B, 0, 3), (filled.data_ptr(), B, H, 4),
                 (filled.data_ptr(), B, H, -1)):
        assert draw(*args, 1, 0, None, _s()) == INVALID, args
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(x, 5.0)) and bool((filled == -7).all()), "a refused call launched something"
    assert gather() == 0 and draw(filled.data_ptr(), B, H, 0, 1, 0, None, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x) and not filled.any(), "mode 0 writes the identity op"


# ------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------
SEED, SUB, NB, HD = 0x1234_5678_9ABC, 4 << 24, 4096, 16


@pytest.fixture(scope="module")
def drawn():
    """draw_augment_ops at B = 4096, H = 16 in the three drawing modes, and cdm_philox_uniform's 3 B values (host)."""
    import cdm_amd
    L = cdm_amd.lib()
    ops = {m: cdm_amd.draw_augment_ops(NB, HD, m, SEED, SUB) for m in ("d4", "shift", "d4+shift", "none")}
    u = torch.empty(3 * NB, device="cuda")
    L.cdm_philox_uniform(u.data_ptr(), 3 * NB, 0.0, 1.0, SEED, SUB, None, _s())
    torch.cuda.synchronize()
    for v in ops.values():
        assert v.dtype == torch.int32 and tuple(v.shape) == (NB, 3) and v.device.type == "cuda"
    return {m: v.cpu() for m, v in ops.items()}, u.cpu().reshape(NB, 3)


def test_draw_follows_the_uniform_stream(drawn):
    ops, u = drawn
    assert u.dtype == torch.float32
    g = (u[:, 0] * torch.tensor(8.0)).to(torch.int32).clamp(max=7)              # fp32 product, truncation, the min
    dy = (u[:, 1] * torch.tensor(float(HD))).to(torch.int32).clamp(max=HD - 1)
    dx = (u[:, 2] * torch.tensor(float(HD))).to(torch.int32).clamp(max=HD - 1)
    assert torch.equal(ops["d4+shift"], torch.stack([g, dy, dx], 1))


def test_draw_coverage(drawn):
    o = drawn[0]["d4+shift"]
    assert int(o.min()) >= 0 and int(o[:, 0].max()) <= 7 and int(o[:, 1:].max()) <= HD - 1
    counts = torch.bincount(o[:, 0].long(), minlength=8)
    print("g counts:", counts.tolist())
    assert counts.numel() == 8 and bool((counts > 0).all())
    assert bool(((counts - 512).abs() <= 127).all()), counts.tolist()
    for col in (1, 2):
        assert sorted(set(o[:, col].tolist())) == list(range(HD))


def test_draw_modes(drawn):
    o = drawn[0]
    both = o["d4+shift"]
    assert not o["none"].any()
    assert not o["d4"][:, 1:].any() and torch.equal(o["d4"][:, 0], both[:, 0])
    assert not o["shift"][:, 0].any() and torch.equal(o["shift"][:, 1:], both[:, 1:])


def test_draw_counter_selects_the_stream():
    """The device counter is added to sub, as in every other draw of the step: a replay draws fresh ops."""
    import cdm_amd
    L = cdm_amd.lib()
    B, H = 257, 16
    got = []
    for k in (0, 5):
        ctr = torch.tensor([k], dtype=torch.int32, device="cuda")
        ops = torch.empty(B, 3, dtype=torch.int32, device="cuda")
        L.cdm_augment_draw(ops.data_ptr(), B, H, 3, 77, SUB, ctr.data_ptr(), _s())
        torch.cuda.synchronize()
        assert torch.equal(ops.cpu(), cdm_amd.draw_augment_ops(B, H, "d4+shift", 77, SUB + k).cpu())
        got.append(ops.cpu())
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------
# Trainer
# ------------------------------------------------------------------------------------------------
NF, H, B, T = 8, 16, 4, 10


def _model(seed=5):
    from cdm_amd import ContextUnet
    torch.manual_seed(seed)
    m = ContextUnet(1, NF, 6, H).cuda().train()
    m.shortcut_source = "device"
    return m


def _batch(seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 1, H, H, generator=g).cuda(), torch.rand(B, 6, generator=g).cuda()


def _inject(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 1, H, H, generator=g).cuda(), torch.randint(1, T + 1, (B,), generator=g).int().cuda(),
            (torch.rand(2 * NF, generator=g) * 2 - 1).cuda())


def _snap(tr):
    torch.cuda.synchronize()
    out = {"flat": tr.flat, "m": tr.m, "v": tr.v, "bn": tr.bnflat, "opt": tr.opt_state, "ctr": tr.ctr}
    return {k: v.cpu().clone() for k, v in out.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def _loss_bits(loss):
    return int(_bits(loss)[0])


def test_fixed_ops_equal_a_plain_trainer_on_the_restated_batch():
    from cdm_amd import Trainer
    x, c = _batch()
    ops = [torch.tensor([[1, 15, 2], [6, 0, 7], [0, 0, 0], [7, 3, 15]]),
           torch.tensor([[4, 1, 0], [3, 9, 9], [5, 15, 1], [2, 0, 4]])]
    injs = [_inject(6), _inject(7)]
    a = Trainer(_model(), 1e-3, T, B, augment="d4+shift")
    la = [_loss_bits(a.step(x, c, inject=inj, aug_ops=o)) for inj, o in zip(injs, ops)]
    assert a.graph is None, "aug_ops runs eagerly"
    assert torch.equal(a.x0.reshape(x.shape), x), "the caller's batch was written"
    A = _snap(a)
    b = Trainer(_model(), 1e-3, T, B, augment="none")
    lb = [_loss_bits(b.step(augment_ref(x, o).cuda(), c, inject=inj)) for inj, o in zip(injs, ops)]
    _same(A, _snap(b))
    assert la == lb
    d = Trainer(_model(), 1e-3, T, B)                                # and the ops matter
    d.step(x, c, inject=injs[0])
    d.step(x, c, inject=injs[1])
    assert not torch.equal(d.flat.cpu(), A["flat"])
    with pytest.raises(ValueError):
        d.step(x, c, aug_ops=ops[0])                                 # built with "none"
    for bad in (ops[0][:3], ops[0].float(), torch.tensor([[8, 0, 0]] * B), torch.tensor([[0, H, 0]] * B)):
        with pytest.raises(ValueError):
            a.step(x, c, aug_ops=bad)
    assert a.steps == 2, "a refused step ran"


@pytest.mark.parametrize("mode", ["d4+shift", "shift"])
def test_graph_replay_equals_eager_with_device_draws(mode):
    from cdm_amd import Trainer, draw_augment_ops
    x, c = _batch()
    runs = []
    for use_graph in (False, True):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, use_graph=use_graph, augment=mode)
        losses, ops = [], []
        for k in range(3):
            losses.append(_loss_bits(tr.step(x, c)))
            ops.append(tr.cur.ops.cpu().clone())
        assert (tr.graph is not None) == use_graph
        assert torch.equal(tr.x0.reshape(x.shape), x), "the caller's batch was written"
        runs.append((_snap(tr), losses, torch.stack(ops)))
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2])
    ops = runs[1][2]
    for k in range(3):                                               # step k draws sub-stream (4 << 24) + k
        assert torch.equal(ops[k], draw_augment_ops(B, H, mode, 9 * 1000003, (4 << 24) + k).cpu())
    assert len({tuple(o.reshape(-1).tolist()) for o in ops}) == 3, "replays draw fresh ops"
    if mode == "shift":
        assert not ops[:, :, 0].any()


def test_resume_continues_bit_identically(tmp_path):
    """The trainers run one after the other: models of one shape share an engine."""
    from cdm_amd import Trainer
    x, c = _batch()
    tr = Trainer(_model(), 1e-3, T, B, seed=9, augment="d4+shift")
    for _ in range(2):
        tr.step(x, c)
    torch.save(tr.state_dict(), tmp_path / "trainer.pt")
    la = [_loss_bits(tr.step(x, c)) for _ in range(2)]
    A = _snap(tr)
    del tr
    sd = torch.load(tmp_path / "trainer.pt", weights_only=True)
    assert sd["augment"] == "d4+shift" and sd["steps"] == 2
    tr2 = Trainer(_model(seed=77), 1e-3, T, B, seed=9, augment="d4+shift")
    tr2.load_state_dict(sd)
    lb = [_loss_bits(tr2.step(x, c)) for _ in range(2)]
    _same(A, _snap(tr2))
    assert la == lb


def test_checkpoint_of_another_mode_raises():
    from cdm_amd import Trainer
    aug = Trainer(_model(), 1e-3, T, B, augment="d4")
    plain = Trainer(_model(), 1e-3, T, B)
    other = Trainer(_model(), 1e-3, T, B, augment="shift")
    sd_aug, sd_plain = aug.state_dict(), plain.state_dict()
    assert sd_plain["augment"] == "none"
    for tr, sd in ((plain, sd_aug), (aug, sd_plain), (other, sd_aug)):
        with pytest.raises(ValueError):
            tr.load_state_dict(sd)
    old = dict(sd_plain)
    del old["augment"]                                               # a checkpoint from before the option
    plain.load_state_dict(old)
    with pytest.raises(ValueError):
        aug.load_state_dict(old)
    aug.load_state_dict(sd_aug)


def test_augment_none_is_the_default_trainer():
    from cdm_amd import Trainer
    x, c = _batch()
    runs = []
    for kw in ({}, {"augment": "none"}):
        tr = Trainer(_model(), 1e-3, T, B, seed=9, **kw)
        losses = [_loss_bits(tr.step(x, c)) for _ in range(3)]
        assert tr.graph is not None and not hasattr(tr.cur, "ops"), "nothing new is allocated"
        runs.append((_snap(tr), losses))
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    aug = Trainer(_model(), 1e-3, T, B, seed=9, augment="d4+shift")  # and a drawing mode walks another trajectory
    for _ in range(3):
        aug.step(x, c)
    assert torch.equal(aug.x0.reshape(x.shape), x), "the caller's batch was written"
    assert not torch.equal(aug.flat.cpu(), runs[0][0]["flat"])
