"""train_diffusion.py --fit-maps with --fit-start / --fit-from-scan: one tiny conditioned run that ends with a fit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")
KEYS = ["best", "history_grad_norm", "history_score", "last_params", "params", "score", "start", "t_grid"]


def _check(z, M, K, iters, start=None):
    assert sorted(z.files) == KEYS
    assert z["params"].shape == z["last_params"].shape == z["start"].shape == (M, K, 6)
    assert z["params"].dtype == np.float32 and z["score"].shape == (M, K) and z["score"].dtype == np.float64
    assert z["history_score"].shape == z["history_grad_norm"].shape == (iters + 1, M, K)
    assert np.isfinite(z["history_score"]).all() and (z["history_score"] > 0).all()
    assert z["t_grid"].tolist() == [4, 8]
    np.testing.assert_array_equal(z["score"], z["history_score"].min(0))
    np.testing.assert_array_equal(z["best"], z["params"][np.arange(M), z["score"].argmin(1)])
    assert (z["params"] >= 0).all() and (z["params"] <= 1).all()
    if start is not None:
        np.testing.assert_array_equal(z["start"], np.broadcast_to(start, (M, K, 6)))


def test_cli_param_fit(tmp_path):
    """T = 8, S = 2 timesteps x R = 2 draws, M = 3 maps: --fit-start with K = 2 starts and columns 0, 3 free (the other
    columns come back as given), then --fit-from-scan 2 out of 3 scanned candidates; param_fit.npz holds the listed keys
    and shapes and the log names the fit.  Bad arguments are refused when they are parsed."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = np.random.default_rng(5)
    maps = g.random((3, 64, 64)).astype(np.float32)
    cand = g.uniform(0.2, 0.8, (3, 6)).astype(np.float32)
    np.save(tmp_path / "maps.npy", maps)
    np.save(tmp_path / "cand.npy", cand)
    np.save(tmp_path / "start.npy", cand[:2])
    base = [sys.executable, CLI, "1e-3", "1", "8", "6", "--synthetic", "150", "--n-feat", "16", "--batch-size", "16",
            "--n-samples", "2"]
    fit = ["--fit-maps", str(tmp_path / "maps.npy"), "--fit-iters", "2", "--fit-lr", "0.05", "--fit-steps", "2",
           "--fit-noise", "2"]
    out_root = tmp_path / "out1"
    r = subprocess.run(base + ["--out-root", str(out_root)] + fit +
                       ["--fit-start", str(tmp_path / "start.npy"), "--fit-free", "0,3", "--fit-weight", "nll"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = out_root / os.listdir(out_root)[0]
    z = np.load(out / "param_fit.npz")
    _check(z, 3, 2, 2, cand[:2])
    np.testing.assert_array_equal(z["last_params"][..., [1, 2, 4, 5]], z["start"][..., [1, 2, 4, 5]])
    assert "Parameter fit of 3 maps from 2 starts, 2 iterations, 2 timesteps x 2 noise draws, weight=nll" in \
        open(out / "timing_and_performance.log").read()
    out_root = tmp_path / "out2"
    r = subprocess.run(base + ["--out-root", str(out_root)] + fit +
                       ["--fit-from-scan", "2", "--scan-maps", str(tmp_path / "maps.npy"), "--scan-candidates",
                        str(tmp_path / "cand.npy"), "--scan-steps", "2", "--scan-noise", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = out_root / os.listdir(out_root)[0]
    z, zs = np.load(out / "param_fit.npz"), np.load(out / "param_scan.npz")
    _check(z, 3, 2, 2)
    np.testing.assert_array_equal(z["start"], cand[np.argsort(zs["score"], axis=1, kind="stable")[:, :2]])
    # refused when the arguments are parsed, before any training
    for extra in (["--fit-start", str(tmp_path / "maps.npy")], ["--fit-from-scan", "2"], [],
                  ["--fit-start", str(tmp_path / "start.npy"), "--fit-free", "0,9"]):
        r = subprocess.run(base[:6] + ["--synthetic", "150", "--out-root", str(tmp_path / "out3")] + fit + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 2 and "--fit-" in r.stderr, (extra, r.stderr[-500:])
