"""Times the continuous VAE's fused training step (vae_train.VAETrainStep) against the autograd step of this same package
(model(c) -> vae_loss -> backward -> FlatAdam.step) on the reference's default model size.

    python scripts/bench_vae.py [--dim 128 --z-dim 64 --batch 64 --frames 1024 --warmup 20 --steps 100]

Each mode runs in a process of its own under its own time limit; every step is bracketed by device events and the MEDIAN step
time is reported.  After the timed window the fused mode takes a few extra steps with every entry-point call bracketed by
events (the per-kernel census).  Prints ONE JSON line.  No GPU: fails, nothing falls back.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(args):
    import torch
    from neural_sound_generation_amd import _lib, models as M, ops
    from neural_sound_generation_amd.optim import FlatAdam
    from neural_sound_generation_amd.vae_train import VAETrainStep, vae_loss
    assert torch.cuda.is_available(), "bench_vae needs cuda:0"
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    model = M.VAE(1, args.dim, args.z_dim).to(dev).train()
    c = torch.rand(args.batch, 1, 80, args.frames, generator=torch.Generator().manual_seed(1234)).to(dev)
    h, w = model.latent_grid(c.shape)
    eps = torch.randn(args.batch, args.z_dim, h, w, generator=torch.Generator().manual_seed(5)).to(dev)
    if args.mode == "fused":
        step = VAETrainStep(model, lr=1e-3)

        def one():
            return step.step(c, eps=eps)
    else:
        opt = FlatAdam(model.parameters(), lr=1e-3)

        def one():
            opt.zero_grad()
            x_tilde, kl = model(c, eps=eps)
            rec = vae_loss(x_tilde, c, torch.zeros((), device=dev))
            (rec + kl).backward()
            opt.step()
            return rec.detach(), kl.detach()
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    events = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rec, kl = one()
        b.record()
        events.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in events)
    out = {"mode": args.mode, "median_ms": statistics.median(ms), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))],
           "rec": float(rec), "kl": float(kl)}
    if args.mode == "fused" and args.census_steps > 0:
        cen = ops.KernelTimer()
        _lib.CENSUS = cen
        for _ in range(args.census_steps):
            one()
        torch.cuda.synchronize()
        _lib.CENSUS = None
        out["census"] = {k: {"per_step": v["launches"] / args.census_steps, "ms_per_step": v["total_ms"] / args.census_steps}
                         for k, v in sorted(cen.summary().items(), key=lambda kv: -kv[1]["total_ms"])}
    print("BENCH_VAE_CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--z-dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--census-steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per mode")
    ap.add_argument("--mode", choices=["fused", "autograd"], default=None, help="(internal: one mode in this process)")
    args = ap.parse_args()
    if args.mode is not None:
        return child(args)
    res = {}
    for mode in ("fused", "autograd"):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
                                                                           ("dim", "z_dim", "batch", "frames", "warmup", "steps", "census_steps")]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
        if p.returncode != 0:       # a fault or an abort ends the benchmark: nothing more is started on the device
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"bench_vae: the {mode} run ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("BENCH_VAE_CHILD ")][-1]
        res[mode] = json.loads(line[len("BENCH_VAE_CHILD "):])
    f, a = res["fused"], res["autograd"]
    print(json.dumps({"bench": "vae_train_step", "dim": args.dim, "z_dim": args.z_dim, "batch": args.batch, "frames": args.frames,
                      "warmup": args.warmup, "steps": args.steps, "fused_median_ms": f["median_ms"], "autograd_median_ms": a["median_ms"],
                      "speedup": a["median_ms"] / f["median_ms"], "fused": f, "autograd": a}))


if __name__ == "__main__":
    main()
