"""Timing of the F0-conditioned decoder's kernels and of the fused step that uses them, each figure the median over windows of
HIP-event times on the launch stream (every call warmed up; a window is a run of whole calls between two events; min and max of
the windows beside it are the run's own spread):
  * kernels: at the bf16 step's latent shape 128 x 20 x 256 x 128 -- nsg_add_cond (rows mode and gather mode, fp32 -> bf16, ReLU,
    both conditioning rows) beside nsg_add_per_clip (fp32 -> bf16), which moves the same tensors; nsg_column_sum (bf16 in) beside
    nsg_clip_colsum; with the bytes each moves and the rate that makes;
  * step: the fused bf16 step at BASELINE configs[2]'s widths (D = 128, K = 512, 7 speakers, B = 128, T = 1024) with g and f0_bins
    against the same step with g only (a model without the table), in one process;
  * f0_bins: nsg_f0_bins for 64 clips of 10 s (862 frames) beside audio.f0 on the same clips.
Without --step this is the driver: every step is a process of its own under `timeout -k 10 <seconds>`, the steps chained so that
the first failure ends the run; --json PATH collects the steps' records.  There is no fallback: without a GPU the steps fail.
    python scripts/f0_cond_timing.py [--json profiles/f0_cond_timing.json]"""
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("kernels", 180), ("step", 240), ("f0_bins", 180))     # (step, its time limit in seconds)
WINDOWS, MIN_WINDOW_S = 9, 0.1


def driver():
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    scratch = tempfile.mkdtemp(prefix="f0_cond_timing_")
    tmp = [os.path.join(scratch, f"{s}.json") for s, _ in STEPS]
    cmd = " && ".join(f"timeout -k 10 {limit} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --step {s} --json {shlex.quote(t)}"
                      for (s, limit), t in zip(STEPS, tmp))
    rc = subprocess.call(cmd, shell=True)
    records = []
    for t in tmp:
        if os.path.exists(t):
            with open(t) as fh:
                records.append(json.load(fh))
            os.remove(t)
    os.rmdir(scratch)
    if rc:
        raise SystemExit(f"f0_cond_timing: a step failed (exit status {rc}); nothing more was started")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(records, fh, indent=1)


def event_time(fn, nbytes=None):
    """Seconds per call from HIP events on the current stream: warm up, size a window to MIN_WINDOW_S, the median of WINDOWS windows."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    times = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    rec = dict(us=statistics.median(times) * 1e6, us_min=min(times) * 1e6, us_max=max(times) * 1e6, calls_per_window=reps)
    if nbytes is not None:
        rec.update(bytes=int(nbytes), tb_per_s=nbytes / statistics.median(times) / 1e12)
    return rec


def step(name):
    import torch
    from neural_sound_generation_amd import audio as Au, models as M, ops
    from neural_sound_generation_amd.train import FusedTrainStep
    if not torch.cuda.is_available():
        raise SystemExit("f0_cond_timing: needs a GPU (cuda:0)")
    dev = torch.device("cuda:0")
    rec = dict(step=name, windows=WINDOWS)
    gen = torch.Generator(device=dev).manual_seed(3)
    if name == "kernels":
        B, H, W, C, K, NB = 128, 20, 256, 128, 512, 33
        n = B * H * W * C
        x = torch.randn(B, H, W, C, device=dev, generator=gen)
        xb = x.to(torch.bfloat16)
        code = torch.randn(K, C, device=dev, generator=gen)
        idx = torch.randint(0, K, (B, H, W), device=dev, generator=gen)
        clip = torch.randn(B, C, device=dev, generator=gen)
        table = torch.randn(NB, C, device=dev, generator=gen)
        bins = torch.randint(0, NB, (B, W), device=dev, generator=gen)
        y = torch.empty(B, H, W, C, dtype=torch.bfloat16, device=dev)
        cs = torch.empty(B, W, C, device=dev)
        rec["shape"] = [B, H, W, C]
        # add_per_clip twice, around the others: its two figures and their windows' min / max are the run's spread
        rec["add_per_clip_f32_bf16"] = event_time(lambda: ops.add_per_clip(x, clip, out=y), 6 * n)
        rec["add_cond_rows_f32_bf16"] = event_time(lambda: ops.add_cond(x, table, bins, clip_rows=clip, relu=True, out=y), 6 * n)
        rec["add_cond_gather_bf16"] = event_time(lambda: ops.add_cond(code, table, bins, idx=idx, clip_rows=clip, relu=True, out=y), 2 * n + 8 * B * H * W)
        rec["add_cond_rows_no_clip_rows"] = event_time(lambda: ops.add_cond(x, table, bins, relu=True, out=y), 6 * n)
        one = torch.zeros_like(bins)
        rec["add_cond_rows_one_bin"] = event_time(lambda: ops.add_cond(x, table, one, clip_rows=clip, relu=True, out=y), 6 * n)
        rec["add_per_clip_f32_bf16_again"] = event_time(lambda: ops.add_per_clip(x, clip, out=y), 6 * n)
        rec["convert_f32_bf16_relu"] = event_time(lambda: ops.convert(x, torch.bfloat16, out=y, relu=True), 6 * n)
        rec["clip_colsum_bf16"] = event_time(lambda: ops.clip_colsum(xb, B), 2 * n)
        rec["column_sum_bf16"] = event_time(lambda: ops.column_sum(xb, out=cs), 2 * n + 4 * B * W * C)
        rec["column_sum_f32"] = event_time(lambda: ops.column_sum(x, out=cs), 4 * n + 4 * B * W * C)
        rec["clip_colsum_of_column_sums"] = event_time(lambda: ops.clip_colsum(cs, B), 4 * B * W * C)
        rec["index_add_rows_of_column_sums"] = event_time(lambda: ops.index_add_rows(bins.view(-1), cs.view(-1, C), NB))
    elif name == "step":
        B, T, D, K, S, NB = 128, 1024, 128, 512, 7, 32
        c = torch.rand(B, 1, 80, T, device=dev, generator=gen)
        g = torch.randint(0, S, (B,), device=dev, generator=gen)
        bins = torch.randint(0, NB + 1, (B, T // 4), device=dev, generator=gen)
        rec.update(B=B, T=T, D=D, K=K, n_speakers=S, n_f0_bins=NB)
        torch.manual_seed(1)
        plain = FusedTrainStep(M.VQVAE(1, D, K, n_speakers=S, compute_dtype=torch.bfloat16).to(dev).train())
        torch.manual_seed(1)
        cond = FusedTrainStep(M.VQVAE(1, D, K, n_speakers=S, n_f0_bins=NB, compute_dtype=torch.bfloat16).to(dev).train())
        rec["step_g_only"] = event_time(lambda: plain.step(c, g))
        rec["step_g_and_f0_bins"] = event_time(lambda: cond.step(c, g, bins))
        rec["step_f0_model_without_bins"] = event_time(lambda: cond.step(c, g))
        rec["step_g_only_again"] = event_time(lambda: plain.step(c, g))
    elif name == "f0_bins":
        import numpy as np
        SR, B, SECONDS = 22050, 64, 10
        n = SECONDS * SR
        t = np.arange(n, dtype=np.float64)
        wav = np.stack([0.3 * sum(0.6 ** h * np.sin(h * 2 * np.pi * np.cumsum((100.0 + 2 * b) * (1.0 + 0.2 * np.sin(2 * np.pi * t / SR)) / SR))
                                  for h in range(1, 7)) for b in range(B)]).astype(np.float32)
        wav = torch.from_numpy(wav).to(dev)
        f0, _ = Au.f0(wav)
        rec.update(clips=B, frames=int(f0.shape[1]), voiced_share=float((f0 > 0).double().mean()))
        aff = Au.f0_affine(Au.logf0_sums(f0), 7.5, 0.2)
        rec["audio_f0"] = event_time(lambda: Au.f0(wav))
        rec["f0_bins"] = event_time(lambda: Au.f0_bins(f0))
        rec["f0_bins_affine_detail"] = event_time(lambda: Au.f0_bins(f0, affine=aff, detail=True))
        rec["logf0_sums_and_affine"] = event_time(lambda: Au.f0_affine(Au.logf0_sums(f0), 7.5, 0.2))
    else:
        raise SystemExit(f"f0_cond_timing: unknown step {name!r}")
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rec, fh)


if __name__ == "__main__":
    if "--step" in sys.argv:
        step(sys.argv[sys.argv.index("--step") + 1])
    else:
        driver()
