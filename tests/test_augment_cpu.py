"""Symmetry augmentation, the part that needs no GPU: the closed-form gather index against the torch restatement for
every op at H = 3 and H = 4, the host validation of ops, the two C prototypes, the Trainer's and the CLI's argument
checks."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from _augment_ref import augment_one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")


def _all_ops(H):
    return [(g, dy, dx) for g in range(8) for dy in range(H) for dx in range(H)]


@pytest.mark.parametrize("H", [3, 4])
def test_source_index_matches_the_torch_restatement(H):
    from cdm_amd import augment_source_index
    x = torch.arange(H * H, dtype=torch.float32).reshape(H, H)      # pixel value == flat index
    ops = _all_ops(H)
    assert len(ops) == 8 * H * H
    for g, dy, dx in ops:
        idx = augment_source_index(H, g, dy, dx)
        assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and idx.shape == (H * H,)
        want = augment_one(x, g, dy, dx).reshape(-1).to(torch.int64).numpy()
        assert np.array_equal(idx, want), (g, dy, dx)
        assert np.array_equal(np.sort(idx), np.arange(H * H)), f"{(g, dy, dx)} is no bijection"


def test_the_eight_g_are_distinct_permutations():
    from cdm_amd import augment_source_index
    perms = {tuple(augment_source_index(3, g, 0, 0).tolist()) for g in range(8)}
    assert len(perms) == 8
    assert tuple(range(9)) == tuple(augment_source_index(3, 0, 0, 0).tolist()), "op (0, 0, 0) is the identity"


def test_source_index_rejects_ops_out_of_range():
    from cdm_amd import augment_source_index
    for bad in ((8, 0, 0), (-1, 0, 0), (0, 4, 0), (0, 0, 4), (0, -1, 0)):
        with pytest.raises(ValueError):
            augment_source_index(4, *bad)


def test_check_augment_ops():
    from cdm_amd import check_augment_ops
    B, H = 3, 5
    good = torch.tensor([[0, 0, 0], [7, 4, 4], [3, 1, 2]])
    out = check_augment_ops(good, B, H)
    assert out.dtype == torch.int32 and out.is_contiguous() and torch.equal(out.long(), good)
    assert check_augment_ops(good.int(), B, H).dtype == torch.int32
    bad = [good[:2], good.reshape(-1), good[:, :2], good.float(), good.double(), good.tolist(),
           torch.tensor([[8, 0, 0], [0, 0, 0], [0, 0, 0]]), torch.tensor([[0, H, 0], [0, 0, 0], [0, 0, 0]]),
           torch.tensor([[0, 0, H], [0, 0, 0], [0, 0, 0]]), torch.tensor([[-1, 0, 0], [0, 0, 0], [0, 0, 0]]),
           torch.tensor([[0, -1, 0], [0, 0, 0], [0, 0, 0]]), torch.tensor([[0, 0, 0], [0, 0, 0], [0, 0, -2]])]
    for ops in bad:
        with pytest.raises(ValueError):
            check_augment_ops(ops, B, H)


def test_header_declares_the_two_entry_points():
    from cdm_amd import _lib
    protos = _lib.parse_header()
    vp, i, ll, ull, ui = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint
    # ops, B, H, mode, seed, sub, sub_dev, stream
    assert protos["cdm_augment_draw"] == [vp, i, i, i, ull, ui, vp, vp]
    # cdm_perturb's list with ops after x and H after HW
    p = list(protos["cdm_perturb"])
    assert protos["cdm_perturb_aug"] == p[:1] + [vp] + p[1:9] + [i] + p[9:]
    assert p[8] is i and p[9] is i                                   # ... HW, T, out ...


def test_trainer_arguments_without_a_gpu():
    from cdm_amd import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["augment"].default == "none"
    assert "aug_ops" in inspect.signature(Trainer.step).parameters
    for bad in ("rot", "D4", "d4+shift ", "", None, 1):
        with pytest.raises(ValueError):                              # before the model is touched
            Trainer(None, 1e-3, 10, 4, augment=bad)


def test_draw_augment_ops_rejects_an_unknown_mode_before_the_library():
    from cdm_amd import draw_augment_ops
    with pytest.raises(ValueError):
        draw_augment_ops(4, 16, "flip", 1)
    with pytest.raises(ValueError):
        draw_augment_ops(0, 16, "d4", 1)


def test_cli_rejects_an_unknown_augment_value(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("_train_diffusion_cli", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(SystemExit) as e:
        cli.main(["1e-3", "1", "20", "--synthetic", "8", "--out-root", str(tmp_path), "--augment", "rot90"])
    assert e.value.code == 2
    assert "invalid choice" in capsys.readouterr().err
