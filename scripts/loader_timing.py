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

--audio: INSTEAD, what pitch-perturbed training costs from a resident AUDIO corpus (data.ResidentMelCorpus.keep_audio), on a voiced
root with audio (--clips of 1 024 .. 2 048 frames, 128 held out) and VQVAE(1, 128, 512, 7 speakers, 32 F0 bins) in bf16 -- no
threshold, every figure is read against its neighbour of the same run:
  kernels, by HIP events, the epoch's batches in turn into rings of outputs larger than the Infinity Cache: nsg_collate_audio at
    128 x 1 024 frames x hop 256, nsg_collate_mels at 128 x 80 x 1 024, and a device copy_ of each one's byte count;
  steps, alternating windows: (a) a fixed batch with fixed bins, (b) the resident loader with f0, (c) the same with audio=True and
    the audio unused, (d) the same with train_conditioned's pitch_perturb=(-4, 4) body, and (e) the host loader
    (get_data_loaders(with_audio=True) + DevicePrefetcher) under the same body, --host-steps consecutive steps;
  (d) by stage, HIP events around each: the loader's three collate launches, the tracker, the pitch marks + synthesis, the mel, the
    step (the host's waits between them fall into the stage they precede).
    python scripts/loader_timing.py --audio [--clips 640] [--host-steps 8] [--out FILE.json]
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
ap.add_argument("--audio", action="store_true", help="the resident audio corpus' measurement instead (see above)")
ap.add_argument("--host-steps", type=int, default=8, help="--audio: timed consecutive steps of the host arm (0: skip it)")
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


def audio_measurement():
    from neural_sound_generation_amd import audio, evaluate as Ev
    NB, FMIN, FMAX, SPEAKERS, HOP, SEMITONES = 32, 65.0, 500.0, 7, Dm.HOP_SIZE, (-4.0, 4.0)
    L = T * HOP
    stat = lambda v: {"best": min(v), "median": float(np.median(v)), "worst": max(v), "all": list(v)}       # noqa: E731

    def timed_windows(fns):
        out = {}
        for _ in range(args.windows):
            for name, fn in fns.items():
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
                out.setdefault(name, []).append(dt / n * 1e3)
        return out

    def event_us(fn, calls):
        fn()
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / calls * 1e3)
        return us

    with tempfile.TemporaryDirectory(prefix="nsg_loader_timing_audio_") as root:
        t0 = time.perf_counter()
        Dm.write_synthetic_data_root(root, n_utts=args.clips, min_frames=T, max_frames=2 * T, n_speakers=SPEAKERS, seed=1, voiced=True)
        print(f"data root: {args.clips} voiced clips with audio written in {time.perf_counter() - t0:.1f} s", flush=True)
        random.seed(1)
        np.random.seed(1)
        src = dict(train=True, test_size=None, test_num_samples=HELD_OUT)
        corpus = Dm.ResidentMelCorpus(Dm.MelSpecDataSource(root, **src), dev)
        t0 = time.perf_counter()
        corpus.keep_audio(Dm.RawAudioDataSource(root, **src))
        torch.cuda.synchronize()
        keep_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        corpus.track_f0()
        torch.cuda.synchronize()
        track_s = time.perf_counter() - t0
        print(f"corpus: {len(corpus)} clips, {corpus.frames.shape[0]} frames: {corpus.frames.numel() * 4 / 1e9:.2f} GB of mels, "
              f"{corpus.audio.numel() * 4 / 1e9:.2f} GB of samples (keep_audio: {keep_s:.1f} s; track_f0() from them, first call: {track_s:.2f} s)", flush=True)
        with_f0 = Dm.ResidentMelLoader(corpus, B, L, train=True, f0=(NB, FMIN, FMAX))
        with_audio = Dm.ResidentMelLoader(corpus, B, L, train=True, f0=(NB, FMIN, FMAX), audio=True)

        # ---- the kernels alone: the entry points called directly
        ep = with_audio.plan_epoch()
        full = [k for k in range(len(ep)) if ep.sizes[k] == B and ep.widths[k] == T]
        plan_dev = torch.from_numpy(ep.plan).to(dev)
        lib, stream = _lib.load(), c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: c_void_p(t.data_ptr())                                                          # noqa: E731
        outs_a = [torch.empty(B, L, device=dev) for _ in range(4)]                                    # 4 x 134 MB
        outs_m = [torch.empty(B, 80, T, device=dev) for _ in range(8)]                                # 8 x 42 MB
        n = 8 * len(full)
        a_calls = [(p(corpus.audio), corpus.audio.numel(), HOP, p(plan_dev[full[i % len(full)]]), B, T, p(outs_a[i % 4]), stream) for i in range(n)]
        m_calls = [(p(corpus.frames), corpus.frames.shape[0], 80, p(plan_dev[full[i % len(full)]]), B, T, p(outs_m[i % 8]), stream) for i in range(n)]

        def run(entry, argv):
            def fn():
                for a in argv:
                    assert entry(*a) == 0
            return fn

        def copies(outs):
            def fn():
                for i in range(n):
                    outs[i % len(outs)].copy_(outs[(i + len(outs) // 2) % len(outs)])
            return fn
        kernels = {}
        for _ in range(2):                                                                            # twice, alternating: the order is not the result
            for name, fn in (("collate_audio", run(lib.nsg_collate_audio, a_calls)), ("copy_of_collate_audio_bytes", copies(outs_a)),
                             ("collate_mels", run(lib.nsg_collate_mels, m_calls)), ("copy_of_collate_mels_bytes", copies(outs_m))):
                kernels.setdefault(name, []).extend(event_us(fn, n))
        assert lib.nsg_collate_audio(*a_calls[-1]) == 0
        rows = ep.plan[full[(n - 1) % len(full)]]
        want = torch.stack([corpus.audio[int(s) * HOP:int(s) * HOP + L] for _, s, _ in rows])
        assert torch.equal(outs_a[(n - 1) % 4], want), "the timed launches did not write the batch"
        nbytes = {"collate_audio": 2 * B * L * 4, "collate_mels": 2 * B * 80 * T * 4}
        nbytes.update({"copy_of_collate_audio_bytes": nbytes["collate_audio"], "copy_of_collate_mels_bytes": nbytes["collate_mels"]})
        for k, v in kernels.items():
            print(f"{k:28s}: best {min(v):7.1f} us, median {float(np.median(v)):7.1f}, spread {min(v):.1f} .. {max(v):.1f} over {len(v)} windows; "
                  f"{nbytes[k] / 1e6:.1f} MB read + written -> {nbytes[k] / min(v) / 1e6:.2f} TB/s at best", flush=True)
        del outs_a, outs_m, want

        # ---- the step, five ways
        torch.manual_seed(1)
        model = M.VQVAE(1, 128, 512, n_speakers=SPEAKERS, n_f0_bins=NB, compute_dtype=torch.bfloat16).to(dev).train()
        step = FusedTrainStep(model, lr=1e-3)
        first = next(iter(with_f0))
        fixed_c, fixed_g, fixed_bins = first[2].unsqueeze(1), first[3], first[5]
        gen = torch.Generator().manual_seed(1)

        def perturbed(batch, marks=None):
            """train.train_conditioned's body under pitch_perturb, audio.perturb_pitch spelt out so that its two halves can be told apart."""
            mark = (lambda: None) if marks is None else (lambda: marks.append(torch.cuda.Event(enable_timing=True)) or marks[-1].record())
            c, g_d, bins = Ev.batch_conditioning("loader_timing", model, batch, dev, audio.f0)
            lens = np.asarray(batch[4]).astype(np.int64)
            wav = batch[0].view(batch[0].shape[0], -1).to(dev).contiguous()
            mark()
            draws = audio.pitch_draws(len(lens), gen, SEMITONES)
            track = audio.f0(wav, sample_rate=22050, lengths=lens)[0]
            mark()
            moved = audio.pitch_shift_psola(wav, track, ratio=draws["ratio"], sample_rate=22050, hop_size=HOP, lengths=lens, fmin=FMIN, fmax=FMAX)
            mark()
            mel = audio.melspectrogram(moved, lengths=lens)
            c_in = mel[:, None, :, :c.shape[3]].contiguous()
            mark()
            step.step(c_in, g_d, f0_bins=bins, target=c)
            mark()
        it_f0, it_audio, it_pert = endless(with_f0), endless(with_audio), endless(with_audio)

        def fed(it):
            def fn():
                b = next(it)
                assert b[2].shape[0] == B and b[2].shape[2] == T
                step.step(b[2].unsqueeze(1), b[3], b[5])
            return fn
        fns = {"a_fixed_batch_fixed_bins": lambda: step.step(fixed_c, fixed_g, fixed_bins), "b_resident_f0": fed(it_f0),
               "c_resident_f0_audio_unused": fed(it_audio), "d_resident_f0_audio_perturbed": lambda: perturbed(next(it_pert))}
        for fn in fns.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        arms = timed_windows(fns)
        for k, v in arms.items():
            print(f"{k:30s}: best {min(v):8.3f} ms/step, median {float(np.median(v)):8.3f}, spread {min(v):.3f} .. {max(v):.3f} over {len(v)} windows", flush=True)

        # ---- (d) by stage
        names = ["loader (collate_mels, collate_f0_bins, collate_audio)", "tracker (audio.f0)", "pitch marks + synthesis (pitch_shift_psola)",
                 "mel (audio.melspectrogram)", "step"]
        stages = {k: [] for k in names}
        for _ in range(4 * args.windows):
            marks = [torch.cuda.Event(enable_timing=True)]
            torch.cuda.synchronize()
            marks[0].record()
            perturbed(next(it_pert), marks)
            torch.cuda.synchronize()
            for k, e0, e1 in zip(names, marks[:-1], marks[1:]):
                stages[k].append(e0.elapsed_time(e1))
        for k, v in stages.items():
            print(f"  {k:56s}: median {float(np.median(v)):7.3f} ms, spread {min(v):.3f} .. {max(v):.3f} over {len(v)} steps", flush=True)
        for it in (it_f0, it_audio, it_pert):
            it.close()

        # ---- (e) the host path under the same body
        host_ms = []
        if args.host_steps > 0:
            workers = args.workers[0] if args.workers else 2
            host = endless(Dm.DevicePrefetcher(Dm.get_data_loaders(root, num_workers=workers, with_audio=True, **kw)["train"], dev))
            for _ in range(2):
                perturbed(next(host))
            for _ in range(args.host_steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                perturbed(next(host))
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host.close()
            print(f"{'e_host_loader_audio_perturbed':30s}: mean {float(np.mean(host_ms)):8.1f} ms/step, best {min(host_ms):.1f}, worst {max(host_ms):.1f} over "
                  f"{len(host_ms)} consecutive steps ({workers} workers; F0 tracked twice: for the bins and for the shift)", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"B": B, "T": T, "hop": HOP, "clips": args.clips, "train_clips": len(corpus), "mel_GB": corpus.frames.numel() * 4 / 1e9,
                       "audio_GB": corpus.audio.numel() * 4 / 1e9, "keep_audio_seconds": keep_s, "track_f0_from_resident_audio_seconds": track_s,
                       "kernel_us": {k: dict(stat(v), bytes=nbytes[k], TBps_best=nbytes[k] / min(v) / 1e6) for k, v in kernels.items()},
                       "ms_per_step": {k: stat(v) for k, v in arms.items()}, "perturbed_step_stage_ms": {k: stat(v) for k, v in stages.items()},
                       "host_loader_audio_perturbed_ms": {"mean": float(np.mean(host_ms)) if host_ms else None, "steps": host_ms}}, f, indent=1)


if args.audio:
    audio_measurement()
    sys.exit(0)


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
