"""Timing of the tempo change and the noise mix (audio.tempo = one nsg_audio_tempo call: a chain launch, one workgroup per clip,
and a render launch; audio.mix_noise = one nsg_audio_mix_noise call: energies, scale, apply): 64 clips of 10 s at 22 050 Hz and
the defaults (segment 1 808, overlap 265, search 324) for the factors 0.85 and 1.15, one such clip alone (the chain's latency),
and the envelope's corner.  Every shape is warmed up, then timed in windows of whole calls that end in a device synchronise; the
figure is the median window.  Beside it: the fp32 numpy restatement (tests/helpers/tempo_ref.py) on 2 s and 10 s of one clip --
the only baseline there is -- with the kernel held to it bit for bit; the mix's bytes per second beside bn_apply's with a
residual (two reads and a write a sample, as the mix's apply pass); and preprocess.process_utterances on a synthetic root with and
without augmented copies.
There is no fallback: without a GPU this fails.    python scripts/tempo_timing.py [--tempo-only] [--json out.json]"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_sound_generation_amd import audio as Au, ops, preprocess
from tests.helpers import tempo_ref as R

if not torch.cuda.is_available():
    raise SystemExit("tempo_timing: needs a GPU (cuda:0)")
dev = torch.device("cuda:0")
WINDOWS, MIN_WINDOW_S = 7, 0.25
SR = 22050


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
S, O, W = Au.tempo_sizes(SR)
for factor in (0.85, 1.15):
    host_s = {}
    for seconds in (2, 10):                            # the restatement on the first seconds of clip 0, and the kernel held to it
        t = time.perf_counter()
        want, n, want_q = R.wsola_f32(host[0, :seconds * SR], None, factor, S, O, W)
        host_s[seconds] = time.perf_counter() - t
        got, _, q = ops.tempo(wav[:1, :seconds * SR].contiguous(), factor, S, O, W, want_positions=True)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(q[0].cpu().numpy(), want_q)
    out, out_lens = ops.tempo(wav, factor, S, O, W)
    full = median_time(lambda: ops.tempo(wav, factor, S, O, W))
    one = median_time(lambda: ops.tempo(wav[:1], factor, S, O, W))
    steps = -(-int(out_lens[0]) // (S - O)) - 1
    rec = dict(shape="defaults", clips=B, seconds=10, factor=factor, segment=S, overlap=O, search=W, steps_per_clip=steps,
               tempo_ms=full[0] * 1e3, tempo_ms_min=full[1] * 1e3, tempo_ms_max=full[2] * 1e3, calls_per_window=full[3], windows=WINDOWS,
               us_per_step_64_clips=full[0] * 1e6 / steps, one_clip_ms=one[0] * 1e3, us_per_step_one_clip=one[0] * 1e6 / steps,
               triples_per_s=B * steps * W * O / full[0], audio_seconds_per_s=B * 10 / full[0],
               host_restatement_s_2s=host_s[2], host_restatement_s_10s=host_s[10], speedup_per_clip_vs_host=host_s[10] / (full[0] / B))
    results.append(rec)
    print(json.dumps(rec), flush=True)

S2, O2, W2 = 8192, 2048, 2048                         # the envelope's corner
full = median_time(lambda: ops.tempo(wav, 1.15, S2, O2, W2))
steps = -(-int(L / 1.15) // (S2 - O2)) - 1
rec = dict(shape="corner", clips=B, seconds=10, factor=1.15, segment=S2, overlap=O2, search=W2, steps_per_clip=steps, tempo_ms=full[0] * 1e3,
           us_per_step_64_clips=full[0] * 1e6 / steps, triples_per_s=B * steps * W2 * O2 / full[0])
results.append(rec)
print(json.dumps(rec), flush=True)

if "--tempo-only" in sys.argv:                         # (an A/B of two builds of csrc/tsm.hip needs no more)
    raise SystemExit(0)

# the mix: 64 clips of 10 s, a 30 s recording; bn_apply with a residual over as many fp32 elements moves the same 12 bytes each
noise = torch.from_numpy((0.1 * np.random.RandomState(1).standard_normal(30 * SR)).astype(np.float32)).to(dev)
level, offset = np.full(B, 0.3), np.arange(B) * 9973
mix_out = torch.empty_like(wav)
mix_call = median_time(lambda: ops.mix_noise(wav, noise, 1.0, level, offset, out=mix_out))          # with the upload of gain, level, offset
on_dev = [torch.ones(B, device=dev), torch.from_numpy(level.astype(np.float32)).to(dev), torch.from_numpy(offset.astype(np.int32)).to(dev)]
assert torch.equal(ops.mix_noise(wav, noise, *on_dev), mix_out)
mix = median_time(lambda: ops.mix_noise(wav, noise, *on_dev, out=mix_out))                           # the three launches alone
C = 128
x = wav[:, :L // C * C].reshape(-1, C).contiguous()
res, y = torch.randn_like(x), torch.empty_like(x)
vec = [torch.rand(C, device=dev) for _ in range(4)]
bn = median_time(lambda: ops.bn_apply(x, *vec, residual=res, out=y))
rec = dict(shape="mix_noise", clips=B, seconds=10, noise_seconds=30, mix_call_with_upload_ms=mix_call[0] * 1e3, mix_ms=mix[0] * 1e3, mix_ms_min=mix[1] * 1e3, mix_ms_max=mix[2] * 1e3,
           mix_bytes_per_s_12_a_sample=12.0 * B * L / mix[0], mix_bytes_per_s_with_the_energy_pass_20_a_sample=20.0 * B * L / mix[0],
           bn_apply_residual_ms=bn[0] * 1e3, bn_apply_bytes_per_s=12.0 * x.numel() / bn[0])
results.append(rec)
print(json.dumps(rec), flush=True)

# preprocessing a synthetic root of 48 utterances of 1 - 4 s, with and without two augmented copies each (tempo and noise)
rs = np.random.RandomState(2)
clips = [voiced_clip(int(SR * rs.uniform(1.0, 4.0)), 100 + i) for i in range(48)]
texts = ["t"] * len(clips)
noise_h = noise.cpu().numpy()
with tempfile.TemporaryDirectory() as tmp:
    def run(copies):
        t = time.perf_counter()
        preprocess.process_utterances(clips, texts, os.path.join(tmp, "c%d" % copies), augment_copies=copies, noise=noise_h if copies else None)
        torch.cuda.synchronize()
        return time.perf_counter() - t
    run(0), run(2)                                     # warm up (tables, allocator, page cache)
    plain = statistics.median(run(0) for _ in range(3))
    aug = statistics.median(run(2) for _ in range(3))
rec = dict(shape="process_utterances", utterances=len(clips), audio_seconds=sum(len(c) for c in clips) / SR, copies=2, plain_s=plain, augmented_s=aug,
           files_ratio=3.0, time_ratio=aug / plain)
results.append(rec)
print(json.dumps(rec), flush=True)
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results, fh, indent=1)
