"""train_diffusion.py --scan-maps / --scan-candidates: one tiny conditioned run that ends with a parameter scan."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "camels-diffusion-model_amd", "train_diffusion.py")


def test_cli_param_scan(tmp_path):
    """T = 8, S = 2 timesteps x R = 2 draws, M = 3 maps, K = 2 candidates: param_scan.npz holds score [M,K], candidates
    [K,6], t_grid [S] and best [M,6] = each map's lowest-score candidate; the log names the scan."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = np.random.default_rng(5)
    maps = g.random((3, 64, 64)).astype(np.float32)
    cand = g.random((2, 6)).astype(np.float32)
    np.save(tmp_path / "maps.npy", maps)
    np.save(tmp_path / "cand.npy", cand)
    out_root = tmp_path / "out"
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "8", "6", "--synthetic", "150", "--n-feat", "16",
                        "--batch-size", "16", "--n-samples", "2", "--out-root", str(out_root),
                        "--scan-maps", str(tmp_path / "maps.npy"), "--scan-candidates", str(tmp_path / "cand.npy"),
                        "--scan-steps", "2", "--scan-noise", "2", "--scan-weight", "nll"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = out_root / os.listdir(out_root)[0]
    z = np.load(out / "param_scan.npz")
    assert sorted(z.files) == ["best", "candidates", "score", "t_grid"]
    assert z["score"].shape == (3, 2) and z["score"].dtype == np.float64
    assert np.isfinite(z["score"]).all() and (z["score"] > 0).all()
    np.testing.assert_array_equal(z["candidates"], cand)
    assert z["t_grid"].tolist() == [4, 8]
    np.testing.assert_array_equal(z["best"], cand[z["score"].argmin(1)])
    assert "Parameter scan of 3 maps under 2 candidates, 2 timesteps x 2 noise draws, weight=nll" in \
        open(out / "timing_and_performance.log").read()
    # a bad file is refused when the arguments are parsed, before any training
    np.save(tmp_path / "bad.npy", cand[:, :5])
    r = subprocess.run([sys.executable, CLI, "1e-3", "1", "8", "6", "--synthetic", "150", "--out-root", str(out_root),
                        "--scan-maps", str(tmp_path / "maps.npy"), "--scan-candidates", str(tmp_path / "bad.npy")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--scan-candidates" in r.stderr
