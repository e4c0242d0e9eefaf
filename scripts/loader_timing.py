"""What feeding the training step from a data root costs, four ways, in ONE process: VQVAE(1, 128, 512) in bf16 with
FusedTrainStep on batches of 128 x 80 x 1024 from a synthetic root of 2 048 clips of 1 024 .. 2 048 frames (every crop is
1 024 frames; 128 clips are held out, so the epoch is 15 full batches); warmed up, device-synchronised, alternating windows:
  (a) one fixed resident batch (what bench.py times),
  (b) the resident loader (data.get_resident_loaders: one collate launch per step),
  (c) data.get_data_loaders(num_workers=2) + DevicePrefetcher,
  (d) the same with num_workers=8
(an epoch of the host loaders starts its worker processes anew, as it does in training: that is part of (c) and (d)).
Then the collate kernel alone, over the epoch's batches in turn and a ring of outputs (more than the Infinity Cache holds, so
nothing is re-read from it): microseconds per launch and its compulsory traffic (B x 80 x T x 4 bytes read, the same written)
over that time, next to a device copy of the same bytes.
Gate: (b) <= 1.05 x (a), best window against best window; the exit status is 1 when it is missed.
    python scripts/loader_timing.py [--windows 5] [--window-s 0.5] [--clips 2048] [--out FILE.json]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
from ctypes import c_void_p

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_sound_generation_amd import _lib, data as Dm, models as M  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--window-s", type=float, default=0.5)
ap.add_argument("--clips", type=int, default=2048)
ap.add_argument("--workers", type=int, nargs="*", default=[2, 8], help="host-loader arms; none: skip them")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
B, T, HELD_OUT = 128, 1024, 128
kw = dict(batch_size=B, max_time_steps=T * Dm.HOP_SIZE, test_size=None, test_num_samples=HELD_OUT)


def endless(loader):
    """Batches of `loader`, epoch after epoch."""
    while True:
        for batch in loader:
            yield batch


with tempfile.TemporaryDirectory(prefix="nsg_loader_timing_") as root:
    t0 = time.perf_counter()
    Dm.write_synthetic_data_root(root, n_utts=args.clips, min_frames=T, max_frames=2 * T, with_audio=False, seed=1)
    print(f"data root: {args.clips} clips written in {time.perf_counter() - t0:.1f} s", flush=True)
    random.seed(1)
    np.random.seed(1)
    t0 = time.perf_counter()
    resident = Dm.get_resident_loaders(root, device=dev, **kw)["train"]
    torch.cuda.synchronize()
    corpus = resident.dataset
    print(f"resident corpus: {len(corpus)} clips, {corpus.frames.shape[0]} frames, {corpus.frames.numel() * 4 / 1e9:.2f} GB, "
          f"read and uploaded in {time.perf_counter() - t0:.1f} s", flush=True)

    torch.manual_seed(1)
    step = FusedTrainStep(M.VQVAE(1, 128, 512, compute_dtype=torch.bfloat16).to(dev).train(), lr=1e-3)
    fixed = next(iter(resident))[2].unsqueeze(1)
    assert tuple(fixed.shape) == (B, 1, 80, T)
    sources = {"b_resident_loader": endless(resident)}
    for k in args.workers:
        sources[f"host_loader_{k}_workers"] = endless(Dm.DevicePrefetcher(Dm.get_data_loaders(root, num_workers=k, **kw)["train"], dev))

    def from_source(it):
        def fn():
            c = next(it)[2]
            assert c.shape[0] == B and c.shape[2] == T
            step.step(c.unsqueeze(1))
        return fn
    fns = {"a_fixed_resident_batch": lambda: step.step(fixed)}
    fns.update({name: from_source(it) for name, it in sources.items()})
    for fn in fns.values():                                    # warm-up: every arm's shapes, the loaders' first epoch start
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    arms = {}
    for w in range(args.windows):
        for name, fn in fns.items():                           # alternating windows
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            while True:
                for _ in range(4):
                    fn()
                n += 4
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.window_s:
                    break
            arms.setdefault(name, []).append(dt / n * 1e3)
    for it in sources.values():                                # ends the host loaders' worker processes before the root goes
        it.close()
    del sources, fns

    # ---- the collate kernel alone: the entry point called directly (the wrapper's host time per call is of the kernel's order)
    ep = resident.plan_epoch()
    full = [k for k in range(len(ep)) if ep.sizes[k] == B and ep.widths[k] == T]
    plan_dev = torch.from_numpy(ep.plan).to(dev)
    outs = [torch.empty(B, 80, T, device=dev) for _ in range(8)]
    nbytes = 2 * B * 80 * T * 4
    lib, stream = _lib.load(), c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 4 * len(full)
    calls = [(c_void_p(corpus.frames.data_ptr()), corpus.frames.shape[0], 80, c_void_p(plan_dev[full[i % len(full)]].data_ptr()), B, T,
              c_void_p(outs[i % len(outs)].data_ptr()), stream) for i in range(n)]

    def collate_all():
        for a in calls:
            assert lib.nsg_collate_mels(*a) == 0

    def copy_all():                                            # the yardstick: a device copy of the same bytes (B x 80 x T read, as many written)
        for i in range(n):
            outs[i % len(outs)].copy_(outs[(i + 3) % len(outs)])
    us, copy_us = [], []
    for w in range(args.windows):
        for fn, into in ((collate_all, us), (copy_all, copy_us)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            into.append(e0.elapsed_time(e1) / n * 1e3)
    want = torch.from_numpy(np.stack([corpus.frames[s:s + T].cpu().numpy().T for _, s, _ in ep.plan[full[(n - 1) % len(full)]]]))
    assert torch.equal(outs[(n - 1) % len(outs)].cpu(), want), "the timed launches did not write the batch"

med = {k: float(np.median(v)) for k, v in arms.items()}
for k, v in arms.items():
    print(f"{k:24s}: best {min(v):8.3f} ms/step, median {med[k]:8.3f}, spread {min(v):.3f} .. {max(v):.3f} over {len(v)} windows")
ratio = min(arms["b_resident_loader"]) / min(arms["a_fixed_resident_batch"])
ok = ratio <= 1.05
print(f"collate_mels alone ({len(full)} batches in turn): best {min(us):.1f} us, spread {min(us):.1f} .. {max(us):.1f}; "
      f"{nbytes / 1e6:.1f} MB compulsory -> {nbytes / min(us) / 1e6:.2f} TB/s; a device copy_ of the same bytes: best {min(copy_us):.1f} us "
      f"-> {nbytes / min(copy_us) / 1e6:.2f} TB/s")
print(f"gate: resident loader / fixed batch = {ratio:.4f} (best windows; medians {med['b_resident_loader'] / med['a_fixed_resident_batch']:.4f}) "
      f"<= 1.05: {'PASS' if ok else 'MISSED'}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"B": B, "T": T, "clips": args.clips, "corpus_GB": corpus.frames.numel() * 4 / 1e9,
                   "ms_per_step": {k: {"best": min(v), "median": med[k], "worst": max(v), "windows": v} for k, v in arms.items()},
                   "collate_us": {"best": min(us), "worst": max(us), "compulsory_bytes": nbytes, "TBps": nbytes / min(us) / 1e6,
                                  "device_copy_same_bytes_us": min(copy_us)},
                   "gate_ratio_best": ratio, "gate": "pass" if ok else "missed"}, f, indent=1)
sys.exit(0 if ok else 1)
