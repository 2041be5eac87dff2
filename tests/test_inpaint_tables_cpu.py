"""Host side of masked (inpainting) sampling: the known-region tables, the input validation and the CLI's argument
errors (no GPU, no library).  The definition is tests/_inpaint_ref.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _inpaint_ref as I
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
N, H = 2, 64


def _fns():
    from cdm_amd.diffusion import check_inpaint, known_tables
    return known_tables, check_inpaint


@pytest.mark.parametrize("T", [10, 100, 1500])
def test_tables_are_fp64_sqrt_rounded_once(T):
    """sab / somab against python-float sqrt of the fp32 ab_t entries (IEEE sqrt on both sides: equal, not close), the
    fp32 tables those values rounded once; the endpoint (1, 0) exact."""
    known_tables, _ = _fns()
    ab_t = R.make_schedule(T)[2]
    sab, somab = known_tables(ab_t)
    assert sab.dtype == somab.dtype == np.float32 and sab.shape == somab.shape == (T + 1,)
    r_sab, r_somab = I.tables(ab_t, torch.float64)
    assert np.array_equal(sab, r_sab.numpy().astype(np.float32))
    assert np.array_equal(somab, r_somab.numpy().astype(np.float32))
    assert np.array_equal(sab, I.tables(ab_t)[0].numpy()) and np.array_equal(somab, I.tables(ab_t)[1].numpy())
    assert sab[0] == 1.0 and somab[0] == 0.0
    assert (sab[1:] < 1).all() and (sab[1:] > 0).all() and (somab[1:] > 0).all() and (somab[1:] < 1).all()
    assert (np.diff(sab) < 0).all() and (np.diff(somab) >= 0).all()    # somab saturates near 1 in fp32 at T = 1500
    # numpy input and a tensor give the same tables; an ab_t whose entry 0 is not 1 still gets the exact endpoint
    assert np.array_equal(known_tables(ab_t.numpy())[0], sab)
    off = ab_t.clone(); off[0] = 0.999
    assert known_tables(off)[0][0] == 1.0 and known_tables(off)[1][0] == 0.0


def test_tables_unit_norm():
    """sab^2 + somab^2 = 1 to fp32 rounding: each table entry is within 2^-24 relative of its exact value, so the
    squares are within 2 * 2^-24 + 2^-48 relative and, the exact squares summing to 1, the sum is within 2^-23 + 2^-48
    of 1 (evaluated in fp64, whose own error is 1e-16)."""
    known_tables, _ = _fns()
    for T in (100, 1500):
        sab, somab = (v.astype(np.float64) for v in known_tables(R.make_schedule(T)[2]))
        dev = np.abs(sab * sab + somab * somab - 1)
        print(f"T = {T}: max |sab^2 + somab^2 - 1| = {dev.max():.3e}")
        assert dev.max() <= 2.0 ** -23 + 2.0 ** -47


def test_tables_bad_input_raises():
    known_tables, _ = _fns()
    ab_t = R.make_schedule(100)[2]
    for bad_value in (float("nan"), 1.5, -0.25, float("inf")):
        bad = ab_t.clone(); bad[50] = bad_value
        with pytest.raises(ValueError):
            known_tables(bad)
    with pytest.raises(ValueError):
        known_tables(torch.ones(1))


def _good():
    g = torch.Generator().manual_seed(3)
    known = torch.rand(N, 1, H, H, generator=g)
    mask = (torch.rand(N, 1, H, H, generator=g) < 0.5).float()
    return known, mask


def test_check_inpaint_accepts():
    _, check = _fns()
    known, mask = _good()
    k, m = check(known, mask, N, H)
    assert k is known and m is mask
    k, m = check(known, mask[:1], N, H, "fresh")
    assert tuple(m.shape) == (1, 1, H, H)
    assert check(None, None, N, H) == (None, None)
    soft = mask * 0.25
    check(known, soft, N, H)
    # known may hold anything where the mask is 0
    holes = known.clone(); holes[mask == 0] = float("nan")
    check(holes, mask, N, H)
    check(known.numpy(), mask.numpy(), N, H)
    check(known.double(), mask.double(), N, H)


def test_check_inpaint_raises():
    _, check = _fns()
    known, mask = _good()
    with pytest.raises(ValueError, match="both"):
        check(known, None, N, H)
    with pytest.raises(ValueError, match="both"):
        check(None, mask, N, H)
    for bad_known in (known[:1], known[:, 0], known[:, :, :32], torch.cat([known, known], 1), known[..., :63]):
        with pytest.raises(ValueError, match="known must have shape"):
            check(bad_known, mask, N, H)
    for bad_mask in (mask[:, 0], mask[0, 0], torch.cat([mask, mask]), mask[..., :63], mask[:, :, :1]):
        with pytest.raises(ValueError, match="mask must have shape"):
            check(known, bad_mask, N, H)
    for v in (-0.01, 1.01, float("nan"), float("inf")):
        bad = mask.clone(); bad[1, 0, 5, 7] = v
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check(known, bad, N, H)
    for v in (float("nan"), float("-inf")):
        bad = known.clone()
        bad[0, 0][mask[0, 0] > 0] = v
        with pytest.raises(ValueError, match="non-finite"):
            check(bad, mask, N, H)
        bad = known.clone(); bad[1, 0, 0, 0] = v          # a soft mask value counts as mask > 0
        soft = mask.clone(); soft[1, 0, 0, 0] = 0.25
        with pytest.raises(ValueError, match="non-finite"):
            check(bad, soft, N, H)
    for mode in ("Fixed", "", None, "repaint"):
        with pytest.raises(ValueError, match="known_noise"):
            check(known, mask, N, H, mode)
        with pytest.raises(ValueError, match="known_noise"):
            check(None, None, N, H, mode)
    with pytest.raises(ValueError, match="in_channels"):
        check(known, mask, N, H, "fixed", 3)
    with pytest.raises(ValueError):
        check(known.long(), mask, N, H)


def _cli():
    spec = importlib.util.spec_from_file_location("_train_diffusion_cli", CLI)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_argument_errors(tmp_path, capsys):
    """The inpaint flags are checked while the arguments are parsed, before any device work: argparse errors (exit 2)."""
    cli = _cli()
    known, mask = _good()
    kp, mp = str(tmp_path / "known.npy"), str(tmp_path / "mask.npy")
    np.save(kp, known.numpy()); np.save(mp, mask.numpy())
    base = ["1e-3", "1", "20", "--synthetic", "8", "--n-samples", str(N), "--out-root", str(tmp_path / "out")]

    def fails(extra, needle):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert needle in err, err

    fails(["--inpaint-known", kp], "go together")
    fails(["--inpaint-mask", mp], "go together")
    fails(["--inpaint-known", kp, "--inpaint-mask", mp, "--inpaint-noise", "repaint"], "invalid choice")
    fails(["--inpaint-known", kp, "--inpaint-mask", str(tmp_path / "missing.npy")], "--inpaint-known / --inpaint-mask")
    fails(["--inpaint-known", kp, "--inpaint-mask", mp, "--n-samples", "3"], "--n-samples is 3")
    bad = str(tmp_path / "bad.npy")
    np.save(bad, known.numpy()[:, :, :32])
    fails(["--inpaint-known", bad, "--inpaint-mask", mp], "known has shape")
    np.save(bad, mask.numpy()[:, 0, :, :60])
    fails(["--inpaint-known", kp, "--inpaint-mask", bad], "mask has shape")
    np.save(bad, mask.numpy() * 2)
    fails(["--inpaint-known", kp, "--inpaint-mask", bad], "[0, 1]")
    np.save(bad, np.full((N, H, H), np.nan, dtype=np.float32))
    fails(["--inpaint-known", bad, "--inpaint-mask", mp], "non-finite")
    assert not (tmp_path / "out").exists()                  # nothing was started


def test_cli_loads_the_accepted_layouts(tmp_path):
    cli = _cli()
    known, mask = _good()
    kp, mp = str(tmp_path / "known.npy"), str(tmp_path / "mask.npy")
    for k_arr, m_arr, mn in ((known.numpy(), mask.numpy(), N), (known.numpy()[:, 0], mask.numpy()[:, 0], N),
                             (known.numpy(), mask.numpy()[0, 0], 1), (known.numpy().astype(np.float64),
                                                                      mask.numpy()[0, 0] > 0.5, 1)):
        np.save(kp, k_arr); np.save(mp, m_arr)
        k, m = cli.load_inpaint(kp, mp, N, H)
        assert k.dtype == m.dtype == torch.float32
        assert tuple(k.shape) == (N, 1, H, H) and tuple(m.shape) == (mn, 1, H, H)
        assert torch.equal(k, known) and torch.equal(m, mask[:mn])
