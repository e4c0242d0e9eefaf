"""Timing of F0 tracking (audio.f0 = one nsg_audio_f0 launch): 64 clips of 10 s at 22 050 Hz and the defaults (window 1 024, hop
256, lags 45 .. 339: 862 frames a clip), and the same at the envelope's largest window and lag range.  Every shape is warmed up,
then timed in windows of whole calls that end in a device synchronise; the figure is the median window.  Beside it: the
one-read-per-pair loop the sliding register window replaces (the diagnostics library's nsg_debug_set_f0_direct, same bits), the
fp32 numpy restatement (tests/helpers/f0_ref.py) on one clip -- the only baseline there is -- and what an
evaluate.test_conversion_f0 batch spends beside its three F0 calls: convert_voice + audio.inv_mel_spectrogram of the same batch,
and the two warpings with their path statistics.
There is no fallback: without a GPU this fails.    python scripts/f0_timing.py [--json out.json]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_sound_generation_amd import _lib, audio as Au, evaluate, models, ops
from tests.helpers import f0_ref as R

if not torch.cuda.is_available():
    raise SystemExit("f0_timing: needs a GPU (cuda:0)")
dev = torch.device("cuda:0")
WINDOWS, MIN_WINDOW_S = 7, 0.25
SR, HOP = 22050, 256


def median_time(fn):
    """Seconds per call: warm up, size a window to at least MIN_WINDOW_S, take the median of WINDOWS windows."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    times = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) / reps)
    return statistics.median(times), min(times), max(times), reps


def voiced_clip(L, seed):
    rs = np.random.RandomState(seed)
    n = np.arange(L, dtype=np.float64)
    phase = 2 * np.pi * np.cumsum(rs.uniform(90.0, 250.0) * (1.0 + 0.2 * np.sin(2 * np.pi * n / SR)) / SR)
    x = sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7)) + 0.02 * rs.standard_normal(L)
    x[int(0.7 * L):int(0.8 * L)] = 0.05 * rs.standard_normal(int(0.8 * L) - int(0.7 * L))
    return (0.3 * x).astype(np.float32)


results = []
B, L = 64, 10 * SR
host = np.stack([voiced_clip(L, b) for b in range(B)])
wav = torch.from_numpy(host).to(dev)
for name, kw, host_seconds in (("defaults", dict(), 10), ("largest", dict(frame_length=2048, fmin=21.533, fmax=500.0), 1)):
    W = kw.get("frame_length", 1024)
    tau_min, tau_max = Au.f0_lags(SR, kw.get("fmin", 65.0), kw.get("fmax", 500.0))
    t = time.perf_counter()                            # the restatement on the first host_seconds of clip 0, and the kernel held to it
    want_f, want_ap = R.yin_f32(host[0, :host_seconds * SR], None, W, HOP, tau_min, tau_max, 0.1, float(SR))
    host_s = time.perf_counter() - t
    cf, cap = Au.f0(wav[:1, :host_seconds * SR].contiguous(), **kw)
    assert np.array_equal(cf[0].cpu().numpy().view(np.uint32), want_f.view(np.uint32)) and np.array_equal(cap[0].cpu().numpy().view(np.uint32), want_ap.view(np.uint32))
    f, ap = Au.f0(wav, **kw)
    full = median_time(lambda: Au.f0(wav, **kw))
    with _lib.use_diag() as lib:                       # the same call through the diagnostics library: its own build of the kernel, then the direct loop
        diag = median_time(lambda: Au.f0(wav, **kw))
        lib.nsg_debug_set_f0_direct(1)
        try:
            fd, apd = Au.f0(wav, **kw)
            assert torch.equal(fd, f) and torch.equal(apd, ap)
            direct = median_time(lambda: Au.f0(wav, **kw))
        finally:
            lib.nsg_debug_set_f0_direct(0)
    T = f.shape[1]
    pairs = B * T * W * tau_max
    rec = dict(shape=name, clips=B, seconds=10, frames=T, window=W, tau_min=tau_min, tau_max=tau_max, voiced_share=float((f > 0).float().mean()),
               f0_ms=full[0] * 1e3, f0_ms_min=full[1] * 1e3, f0_ms_max=full[2] * 1e3, calls_per_window=full[3], windows=WINDOWS,
               pairs_per_s=pairs / full[0], frames_per_s=B * T / full[0], diag_build_ms=diag[0] * 1e3, direct_loop_ms=direct[0] * 1e3,
               host_restatement_s=host_s, host_seconds_of_audio=host_seconds, host_pairs_per_s=len(want_f) * W * tau_max / host_s)
    results.append(rec)
    print(json.dumps(rec), flush=True)

# the share of a test_conversion_f0 batch: the conversion and inversion of 64 clips of 10 s against the three F0 calls and the warpings
model = models.VQVAE(1, 256, 512, n_speakers=4).to(dev).eval()
lens = np.full(B, L, dtype=np.int64)
mel = Au.melspectrogram(wav, lengths=lens)
Tc = mel.shape[2] // 4 * 4
g = torch.arange(B, dtype=torch.int64) % 4
angles = torch.rand(B, Tc, 513, device=dev, generator=torch.Generator(dev).manual_seed(0))
_, conv = evaluate.convert_voice(model, mel[:, :, :Tc].contiguous(), g)
wav_c = Au.inv_mel_spectrogram(conv.squeeze(1), angles0=angles)
frames, frames_c = np.full(B, mel.shape[2], dtype=np.int32), np.full(B, Tc, dtype=np.int32)


def three_f0():
    Au.f0(wav_c)
    Au.f0(wav, lengths=lens)
    Au.f0(wav, lengths=lens)


def two_warpings():
    cep_t = Au.mel_cepstra(mel, frames)
    for m, fr, wv in ((conv, frames_c, wav_c), (mel, frames, wav)):
        cost, steps, path = ops.dtw(Au.mel_cepstra(m, fr), cep_t, fr, frames, want_path=True)
        ops.f0_path_stats(f[:, :m.shape[-1]].contiguous(), f, path, steps)


t_conv = median_time(lambda: evaluate.convert_voice(model, mel[:, :, :Tc].contiguous(), g))[0]
t_inv = median_time(lambda: Au.inv_mel_spectrogram(conv.squeeze(1), angles0=angles))[0]
t_mel = median_time(lambda: (Au.melspectrogram(wav, lengths=lens), Au.melspectrogram(wav, lengths=lens)))[0]
t_f0, t_warp = median_time(three_f0)[0], median_time(two_warpings)[0]
total = t_conv + t_inv + t_mel + t_f0 + t_warp
rec = dict(conversion_f0_batch=dict(clips=B, frames=int(mel.shape[2]), dim=256, codes=512, griffin_lim_iters=Au.GRIFFIN_LIM_ITERS),
           two_melspectrograms_ms=t_mel * 1e3, convert_voice_ms=t_conv * 1e3, inv_mel_spectrogram_ms=t_inv * 1e3, three_f0_ms=t_f0 * 1e3,
           two_warpings_with_stats_ms=t_warp * 1e3, f0_share=t_f0 / total)
results.append(rec)
print(json.dumps(rec), flush=True)
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results, fh, indent=1)
