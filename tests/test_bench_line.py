"""bench.py's record must be ONE short JSON line: the driver keeps only the tail of stdout (round 2's 20 KB line lost its
head -- value, roofline, cpu_baseline -- and the round was recorded as unmeasured)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _canned(n_other):
    roof = {"bound": "mfma", "kernel": "patch_gemm_kernel (gemm_patch.hip: conv forward + data gradient, bf16)", "achieved": 926.91,
            "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.3707, "traffic": 0.706, "traffic_unit": "GB/launch (rocprofv3 PMC, profiles/)",
            "launches": 240, "avg_launch_ms": 0.2626, "gflop_per_launch": 243.403, "share_of_step": 0.37, "step_frac": 0.2246}
    cpu = {"value": 4021.3, "unit": "mel-frames/s", "cores": 16, "kind": "port",
           "sample": "oracle train_step, 4 clips x 80x1024, 1 warm-up + 3 timed steps (1018 ms/step)"}
    other = {"dtype": "f32", "value": 2741234.5, "ms_per_step": 47.812, "frac": 0.7912, "step_frac": 0.6353}
    oc = [{"workload": "configs[3] D=256 K=8192", "dtype": "bf16", "clips": 16, "value": 2775123.4, "ms_per_step": 5.904, "step_frac": 0.1813,
           "vq_frac": 0.1234, "vq_share": 0.1899}] * n_other
    return dict(value=15401234.5, ms_per_step=8.511, world=1, steps=20, warmup=5, dtype="bf16", D=128, K=512, B=128, T=1024,
                roof=roof, cpu=cpu, other=other, other_configs=oc)


def test_line_is_short_and_complete():
    text = bench.build_line(**_canned(4))
    assert "\n" not in text and len(text) < 3072, len(text)
    line = json.loads(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "other_mode", "other_configs"):
        assert key in line, key
    assert line["vs_baseline"] is None and line["scaling"] == "weak" and line["higher_is_better"] is True
    for key in ("workload", "clips_per_gpu", "global_batch", "frames", "parallelism"):
        assert key in line["config"], key
    assert "model" not in line["config"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in line["roofline"], key
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in line["cpu_baseline"], key
    assert len(line["other_configs"]) == 4


def test_line_sheds_the_optional_part_rather_than_grow():
    text = bench.build_line(**_canned(40))
    assert len(text) < 3072
    line = json.loads(text)
    assert line["other_configs"] is None and line["roofline"]["frac"] == 0.3707 and line["cpu_baseline"]["cores"] == 16


def test_kernel_tables_go_to_a_side_file_not_stdout(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    path = bench.write_kernel_tables({"configs[1] bf16 B=128": [{"kernel": "patch_gemm 3x3", "us_per_launch": 186.7, "frac": 0.41}]})
    assert os.path.dirname(path) == str(tmp_path) and json.load(open(path))
    out = capsys.readouterr()
    assert out.out == "" and "patch_gemm 3x3" in out.err


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    import numpy as np
    rng = np.random.default_rng(0)
    arrays = {"losses": np.array([1.0, 2.0, 2.0]), "big": rng.standard_normal(50_000).astype(np.float32),
              "idx": np.arange(30_000, dtype=np.float64), "count": np.array(7.0)}
    whole = bench.write_outputs(str(tmp_path / "a"), dict(arrays), limit=10 ** 7)
    for p in whole:
        a = arrays[os.path.basename(p)[:-4]]
        assert np.load(p).shape == a.shape and np.array_equal(np.load(p), a)      # 0-d arrays stay 0-d
    limit = 120_000
    pa = bench.write_outputs(str(tmp_path / "b"), dict(arrays), limit=limit)
    pb = bench.write_outputs(str(tmp_path / "c"), dict(arrays), limit=limit)
    got = {os.path.basename(p)[:-4]: np.load(p) for p in pa}
    assert sum(a.nbytes for a in got.values()) <= limit
    assert np.array_equal(got["losses"], arrays["losses"])
    for name in ("big", "idx"):
        assert got[name].dtype == arrays[name].dtype and 0 < got[name].size < arrays[name].size
        assert np.isin(got[name], arrays[name]).all()
    assert (np.diff(got["idx"]) > 0).all()                       # sampled positions kept in order
    for p, q in zip(pa, pb):
        assert np.array_equal(np.load(p), np.load(q))            # the same positions on every run


def test_dump_arrays_are_float32_or_float64():
    import torch

    class Step:
        last_indices = torch.tensor([[3, 1], [0, 2]])

    model = torch.nn.Sequential(torch.nn.Linear(2, 2).to(torch.bfloat16), torch.nn.BatchNorm1d(2))
    out = bench.step_outputs(Step(), model, (torch.tensor(0.5), torch.tensor(0.25, dtype=torch.float64), torch.tensor(0.25)))
    assert out["losses"].dtype.name == "float64" and out["losses"].tolist() == [0.5, 0.25, 0.25]
    assert out["indices"].dtype.name == "float64" and out["indices"].tolist() == [3, 1, 0, 2]
    assert out["state.0.weight"].dtype.name == "float32" and out["state.1.num_batches_tracked"].dtype.name == "float64"
    assert set(out) == {"losses", "indices"} | {"state." + k for k in model.state_dict()}
