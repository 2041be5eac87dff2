"""The plain benchmark run on the GPU: `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` times K train steps
alone and writes what the last one computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_k_steps_and_dumps_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = lines[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["train_step_stats"]["steps"] == 3
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["ms_per_step"] > 0 and abs(out["value"] - 256 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    # only the train-step figure: none of the --full legs ran
    assert out["full"] is False
    assert not {"sample", "roofline", "configs", "reference_logged_workloads", "cpu_baseline"} & set(out)
    files = sorted(os.listdir(tmp_path / "dump"))
    assert "loss.npy" in files and "bn_running_stats.npy" in files
    total = 0
    arrays = {}
    for f in files:
        assert f.endswith(".npy")
        a = arrays[f[:-4]] = np.load(tmp_path / "dump" / f)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), f
        total += os.path.getsize(tmp_path / "dump" / f)
    assert total <= 64 * 2 ** 20
    assert arrays["loss"].shape == (1,) and arrays["loss"][0] == np.float32(out["final_loss"])
    params = {k[len("param."):] for k in arrays if k.startswith("param.")}
    grads = {k[len("grad."):] for k in arrays if k.startswith("grad.")}
    assert params == grads and "up0.0.weight" in params and "out.3.bias" in params
    assert arrays["param.out.3.bias"].shape == (1,)                     # small tensors whole,
    assert arrays["param.up0.0.weight"].shape == arrays["grad.up0.0.weight"].shape == (1 << 20,)   # large ones sampled
    assert np.abs(arrays["grad.up0.0.weight"]).max() > 0
