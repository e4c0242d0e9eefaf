"""What feeding an F0-CONDITIONED training step costs, from a resident F0 track and from the host path, in ONE process:
VQVAE(1, 128, 512, 7 speakers, 32 F0 bins) in bf16 with FusedTrainStep on batches of 128 x 80 x 1024 from a synthetic VOICED root
(write_synthetic_data_root(voiced=True)) of clips of 1 024 .. 2 048 frames, 128 of them held out; every crop is 1 024 frames.
Warmed up, device-synchronised, alternating windows -- no threshold: each figure is read against its neighbour of the same run:
  (a) the fused step on one fixed batch with fixed bins;
  (b) the step fed by the resident loader WITHOUT f0 (its c and g; the fixed bins);
  (c) the step fed by the resident loader WITH f0 (its six-tuples): expected at (b) plus the collate_f0_bins launch, within the
      spread of (a)'s windows;
  (d) the step fed by data.get_data_loaders(with_audio=True) with F0 tracked per step (evaluate.batch_conditioning: what
      train.train_conditioned does with a five-tuple): a few consecutive steps after two of warm-up; their MEAN is the rate
      (the workers' queue makes single steps short or long).
Then nsg_collate_f0_bins alone (the epoch's batches in turn) beside nsg_f0_bins on an already gathered (128, 1024) batch, by HIP
events, and the one-off cost of ResidentMelCorpus.track_f0 for the corpus (wall clock, synchronised).
    python scripts/resident_f0_timing.py [--windows 5] [--window-s 0.5] [--clips 640] [--host-steps 16] [--out FILE.json]
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

from neural_sound_generation_amd import _lib, audio, data as Dm, evaluate as Ev, models as M  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--window-s", type=float, default=0.5)
ap.add_argument("--clips", type=int, default=640)
ap.add_argument("--host-steps", type=int, default=16, help="timed consecutive steps of the host arm (0: skip it)")
ap.add_argument("--workers", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
B, T, HELD_OUT, NB, FMIN, FMAX, SPEAKERS = 128, 1024, 128, 32, 65.0, 500.0, 7
kw = dict(batch_size=B, max_time_steps=T * Dm.HOP_SIZE, test_size=None, test_num_samples=HELD_OUT)


def endless(loader):
    """Batches of `loader`, epoch after epoch."""
    while True:
        for batch in loader:
            yield batch


def windows(fns, n_windows, window_s):
    """Alternating windows of whole calls, device-synchronised at both ends -> {name: [ms per call, ...]}."""
    out = {}
    for _ in range(n_windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            while True:
                for _ in range(4):
                    fn()
                n += 4
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= window_s:
                    break
            out.setdefault(name, []).append(dt / n * 1e3)
    return out


def event_us(fn, calls, n_windows):
    """Microseconds per call by HIP events on the current stream: fn() issues `calls` calls; one warm-up run, then the windows."""
    fn()
    us = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / calls * 1e3)
    return us


with tempfile.TemporaryDirectory(prefix="nsg_resident_f0_timing_") as root:
    t0 = time.perf_counter()
    Dm.write_synthetic_data_root(root, n_utts=args.clips, min_frames=T, max_frames=2 * T, n_speakers=SPEAKERS, seed=1, voiced=True)
    print(f"batches per epoch: {(args.clips - HELD_OUT) // B} (the epoch's plan is drawn and uploaded once per epoch)", flush=True)
    print(f"data root: {args.clips} voiced clips written in {time.perf_counter() - t0:.1f} s", flush=True)
    random.seed(1)
    np.random.seed(1)
    plain = Dm.get_resident_loaders(root, device=dev, **kw)["train"]
    corpus = plain.dataset
    src = dict(train=True, test_size=None, test_num_samples=HELD_OUT)
    audio_source = Dm.RawAudioDataSource(root, **src)
    corpus.track_f0(audio_source)                                   # (warm-up: the tracker's first launches, the page cache)
    torch.cuda.synchronize()
    track_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        corpus.track_f0(audio_source)
        torch.cuda.synchronize()
        track_s.append(time.perf_counter() - t0)
    seconds = float(np.sum(corpus.lengths)) / 22050.0
    voiced_share = float((corpus.f0 > 0).double().mean())
    print(f"corpus: {len(corpus)} clips, {corpus.frames.shape[0]} frames, {seconds / 60:.1f} min of audio, {voiced_share:.2f} of the frames voiced; "
          f"track_f0 (read, upload, YIN, sums): best {min(track_s):.2f} s of {[round(v, 2) for v in track_s]}", flush=True)
    with_f0 = Dm.ResidentMelLoader(corpus, B, T * Dm.HOP_SIZE, train=True, f0=(NB, FMIN, FMAX))

    torch.manual_seed(1)
    model = M.VQVAE(1, 128, 512, n_speakers=SPEAKERS, n_f0_bins=NB, compute_dtype=torch.bfloat16).to(dev).train()
    step = FusedTrainStep(model, lr=1e-3)
    first = next(iter(with_f0))
    fixed_c, fixed_g, fixed_bins = first[2].unsqueeze(1), first[3], first[5]
    assert tuple(fixed_c.shape) == (B, 1, 80, T) and tuple(fixed_bins.shape) == (B, T // 4)
    it_plain, it_f0 = endless(plain), endless(with_f0)

    def from_plain():
        b = next(it_plain)
        step.step(b[2].unsqueeze(1), b[3], fixed_bins)

    def from_f0():
        b = next(it_f0)
        step.step(b[2].unsqueeze(1), b[3], b[5])
    fns = {"a_fixed_batch_fixed_bins": lambda: step.step(fixed_c, fixed_g, fixed_bins), "b_resident_loader": from_plain,
           "c_resident_loader_with_f0": from_f0}
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    arms = windows(fns, args.windows, args.window_s)
    it_plain.close()
    it_f0.close()

    # ---- (d) the host path: audio in the batch, F0 tracked per step
    host_ms = []
    if args.host_steps > 0:
        host = endless(Dm.DevicePrefetcher(Dm.get_data_loaders(root, num_workers=args.workers, with_audio=True, **kw)["train"], dev))

        def from_host():
            c, g, bins = Ev.batch_conditioning("resident_f0_timing", model, next(host), dev, audio.f0)
            assert c.shape[0] == B and c.shape[3] == T
            step.step(c, g, bins)
        for _ in range(2):
            from_host()
        for _ in range(args.host_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            from_host()
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        host.close()

    # ---- the kernels alone: the entry points called directly
    ep = with_f0.plan_epoch()
    full = [k for k in range(len(ep)) if ep.sizes[k] == B and ep.widths[k] == T]
    plan_dev = torch.from_numpy(ep.plan).to(dev)
    lib, stream = _lib.load(), c_void_p(torch.cuda.current_stream().cuda_stream)
    W = T // 4
    outs = [torch.empty(B, W, dtype=torch.int64, device=dev) for _ in range(8)]
    rows = torch.empty(B, T, device=dev)
    n = 64
    p = lambda t: c_void_p(t.data_ptr())                                                          # noqa: E731
    calls = [(p(corpus.f0), corpus.f0.shape[0], p(plan_dev[full[i % len(full)]]), None, p(outs[i % 8]), None, None, B, T, W, NB, FMIN, FMAX, stream)
             for i in range(n)]
    with_rows = [a[:6] + (p(rows),) + a[7:] for a in calls]
    gathered = [(p(rows), None, None, p(outs[i % 8]), None, B, T, W, NB, FMIN, FMAX, stream) for i in range(n)]

    def run(entry, argv):
        def fn():
            for a in argv:
                assert entry(*a) == 0
        return fn
    assert lib.nsg_collate_f0_bins(*with_rows[-1]) == 0                                           # the gathered rows of the last timed plan
    kernels = {"collate_f0_bins": event_us(run(lib.nsg_collate_f0_bins, calls), n, args.windows),
               "collate_f0_bins_with_f0_out": event_us(run(lib.nsg_collate_f0_bins, with_rows), n, args.windows),
               "f0_bins_on_gathered_rows": event_us(run(lib.nsg_f0_bins, gathered), n, args.windows)}
    want = outs[(n - 1) % 8].clone()
    assert lib.nsg_collate_f0_bins(*calls[-1]) == 0
    assert torch.equal(outs[(n - 1) % 8], want) and int(want.max()) > 0, "the two kernels disagree on the timed batch"

med = {k: float(np.median(v)) for k, v in arms.items()}
for k, v in arms.items():
    print(f"{k:28s}: best {min(v):8.3f} ms/step, median {med[k]:8.3f}, spread {min(v):.3f} .. {max(v):.3f} over {len(v)} windows")
if host_ms:
    # (the mean is the rate: a step served from the workers' queue is short, the one that waits for them pays for it)
    print(f"{'d_host_loader_audio_tracking':28s}: mean {float(np.mean(host_ms)):8.1f} ms/step, best {min(host_ms):.1f}, median {float(np.median(host_ms)):.1f}, "
          f"worst {max(host_ms):.1f} over {len(host_ms)} consecutive steps ({args.workers} workers)")
for k, v in kernels.items():
    print(f"{k:28s}: best {min(v):7.2f} us, median {float(np.median(v)):7.2f}, spread {min(v):.2f} .. {max(v):.2f}")
extra = med["c_resident_loader_with_f0"] - med["b_resident_loader"]
spread_a = max(arms["a_fixed_batch_fixed_bins"]) - min(arms["a_fixed_batch_fixed_bins"])
print(f"(c) - (b) = {extra * 1e3:.1f} us (medians); collate_f0_bins alone {float(np.median(kernels['collate_f0_bins'])):.1f} us; "
      f"spread of (a)'s windows {spread_a * 1e3:.1f} us", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"B": B, "T": T, "n_f0_bins": NB, "clips": args.clips, "train_clips": len(corpus), "batches_per_epoch": len(corpus) // B, "corpus_frames": int(corpus.frames.shape[0]),
                   "audio_minutes": seconds / 60, "voiced_share": voiced_share, "track_f0_seconds": track_s,
                   "ms_per_step": {k: {"best": min(v), "median": med[k], "worst": max(v), "windows": v} for k, v in arms.items()},
                   "host_loader_audio_tracking_ms": {"workers": args.workers, "mean": float(np.mean(host_ms)) if host_ms else None, "steps": host_ms},
                   "kernel_us": {k: {"best": min(v), "median": float(np.median(v)), "worst": max(v)} for k, v in kernels.items()},
                   "c_minus_b_us": extra * 1e3, "spread_of_a_us": spread_a * 1e3}, f, indent=1)
