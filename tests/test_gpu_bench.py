"""bench.py end to end on the GPU, at a tiny size: a plain run prints the headline line and nothing it does not need, and
--dump-outputs writes what the timed path computed in its last step (bit for bit the same steps taken here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_sound_generation_amd import models as M  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep  # noqa: E402


def test_plain_run_and_dumped_outputs(tmp_path):
    D, K, B, T, steps, warmup = 32, 64, 2, 256, 3, 1
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dtype", "f32", "--dim", str(D), "--z-dim", str(K), "--batch", str(B), "--frames", str(T), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)   # a fresh process of its own
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "mel-frames/s"
    assert abs(line["value"] - B * T / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for key in ("roofline", "cpu_baseline", "other_mode", "other_configs"):     # --full only
        assert line[key] is None, key
    assert not os.path.exists(os.path.join(str(tmp_path), "bench_kernels.json"))

    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    torch.manual_seed(1)                                   # what bench.py does, taken here
    model = M.VQVAE(1, D, K).to("cuda:0").train()
    step = FusedTrainStep(model, lr=1e-3, beta=1.0)
    c = torch.rand(B, 1, 80, T, generator=torch.Generator().manual_seed(1234)).to("cuda:0")
    for _ in range(warmup + steps):
        losses = step.step(c)
    want = {"losses": np.array([float(x.item()) for x in losses]), "indices": step.last_indices.reshape(-1).cpu().numpy()}
    want.update({"state." + k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    assert set(got) == set(want)
    for k, v in want.items():                              # the fp32 step is bitwise reproducible (test_gpu_model.py)
        assert got[k].shape == v.shape and np.array_equal(got[k], v), k
