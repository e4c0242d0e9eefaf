"""Timing of the path finder over YIN candidates (audio.f0_track = nsg_audio_f0_candidates, then nsg_f0_viterbi) on the batch
scripts/f0_timing.py uses: 64 clips of 10 s at 22 050 Hz and the defaults (window 1 024, hop 256, lags 45 .. 339: 862 frames a
clip).  Every call is warmed up, then timed in windows of whole calls that end in a device synchronise; the figure is the median
window.  In one session, so that the figures can be set against one another: nsg_audio_f0, nsg_audio_f0_candidates, nsg_f0_viterbi
(per clip and per frame step: the clips run side by side, one wave each, so the launch's time is a clip's), the fp32 numpy
restatement of the path finder on one clip, and what an evaluate.test_conversion_f0(tracker="viterbi") batch spends in its three
f0_track calls beside its other stages.  The device results are held to the restatements first.
--lib PATH times nsg_audio_f0 alone through another build of the library (the commit before a change to csrc/f0.hip, say) in
windows that alternate with this build's, and checks that the two return the same bits.
There is no fallback: without a GPU this fails.    python scripts/f0_track_timing.py [--json out.json] [--lib other/libnsg.so]"""
import ctypes
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_sound_generation_amd import _lib, audio as Au, evaluate, models, ops
from tests.helpers import f0_track_ref as K

if not torch.cuda.is_available():
    raise SystemExit("f0_track_timing: needs a GPU (cuda:0)")
dev = torch.device("cuda:0")
WINDOWS, MIN_WINDOW_S = 7, 0.25
SR, HOP, W = 22050, 256, 1024


def windows(fns):
    """Seconds per call of each function: warm up, size a window to at least MIN_WINDOW_S, then WINDOWS rounds of one window of
    each function in turn -> [(median, min, max, calls per window)]."""
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps.append(max(1, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6))))
    times = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps[k]):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / reps[k])
    return [(statistics.median(ts), min(ts), max(ts), r) for ts, r in zip(times, reps)]


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
tau_min, tau_max = Au.f0_lags(SR, 65.0, 500.0)
top = math.log2(SR / tau_min)
costs = tuple(Au.F0_TRACK_COSTS[k] for k in ("octave_cost", "jump_cost", "vuv_cost", "unvoiced_cost"))
T = 1 + L // HOP

if "--lib" in sys.argv:
    other = ctypes.CDLL(sys.argv[sys.argv.index("--lib") + 1])
    other.nsg_audio_f0.restype, other.nsg_audio_f0.argtypes = _lib._SIGS["nsg_audio_f0"]
    f, ap = ops.f0(wav, W, HOP, tau_min, tau_max, 0.1, float(SR))
    fo, apo = torch.empty_like(f), torch.empty_like(ap)

    def other_f0():
        rc = other.nsg_audio_f0(ops._p(wav), None, ops._p(fo), ops._p(apo), B, L, W, HOP, tau_min, tau_max, 0.1, float(SR), ops._stream())
        assert rc == 0, rc

    other_f0()
    assert torch.equal(fo, f) and torch.equal(apo, ap), "the two builds of nsg_audio_f0 differ"
    (this, that) = windows([lambda: ops.f0(wav, W, HOP, tau_min, tau_max, 0.1, float(SR), out=(f, ap)), other_f0])
    rec = dict(ab="nsg_audio_f0, this build against --lib, alternating windows", clips=B, frames=T, same_bits=True, this_ms=this[0] * 1e3,
               this_ms_min=this[1] * 1e3, this_ms_max=this[2] * 1e3, other_ms=that[0] * 1e3, other_ms_min=that[1] * 1e3,
               other_ms_max=that[2] * 1e3, ratio=this[0] / that[0], calls_per_window=this[3], windows=WINDOWS)
    results.append(rec)
    print(json.dumps(rec), flush=True)

# the device results against the restatements, on the first second of clip 0 and as row 0 of the batch
cand = ops.f0_candidates(wav, W, HOP, tau_min, tau_max, float(SR))
want = K.candidates_f32(host[0, :SR], None, W, HOP, tau_min, tau_max, float(SR))
short = ops.f0_candidates(wav[:1, :SR].contiguous(), W, HOP, tau_min, tau_max, float(SR))
for g, w in zip((short[0], short[1], short[3]), (want[0], want[1], want[3])):
    assert np.array_equal(g[0].cpu().numpy().view(np.uint32), w.view(np.uint32))
cf, ca, cl, cnt = cand
track = ops.f0_viterbi(cl, ca, cf, cnt, top, *costs)
h = [t[0].cpu().numpy() for t in (cl, ca, cf, cnt)]
t0 = time.perf_counter()
ws, wc, wf, wa = K.viterbi_f32(*h, None, top, *costs)
host_s = time.perf_counter() - t0
assert np.array_equal(track[0][0].cpu().numpy(), ws) and np.array_equal(track[2][0].cpu().numpy().view(np.uint32), wf.view(np.uint32))

f, ap = ops.f0(wav, W, HOP, tau_min, tau_max, 0.1, float(SR))
t_f0, t_cand, t_vit, t_track = windows([lambda: ops.f0(wav, W, HOP, tau_min, tau_max, 0.1, float(SR), out=(f, ap)),
                                        lambda: ops.f0_candidates(wav, W, HOP, tau_min, tau_max, float(SR), out=cand),
                                        lambda: ops.f0_viterbi(cl, ca, cf, cnt, top, *costs, out=track),
                                        lambda: Au.f0_track(wav)])
rec = dict(clips=B, seconds=10, frames=T, window=W, tau_min=tau_min, tau_max=tau_max, mean_candidates=float(cnt.float().mean()),
           voiced_share_yin=float((f > 0).float().mean()), voiced_share_track=float((track[2] > 0).float().mean()),
           f0_ms=t_f0[0] * 1e3, f0_ms_min=t_f0[1] * 1e3, f0_ms_max=t_f0[2] * 1e3,
           candidates_ms=t_cand[0] * 1e3, candidates_ms_min=t_cand[1] * 1e3, candidates_ms_max=t_cand[2] * 1e3, candidates_over_f0=t_cand[0] / t_f0[0],
           viterbi_ms=t_vit[0] * 1e3, viterbi_ms_min=t_vit[1] * 1e3, viterbi_ms_max=t_vit[2] * 1e3, viterbi_us_per_clip=t_vit[0] * 1e6,
           viterbi_ns_per_frame_step=t_vit[0] * 1e9 / T, f0_track_ms=t_track[0] * 1e3, host_viterbi_f32_s_per_clip=host_s, windows=WINDOWS)
results.append(rec)
print(json.dumps(rec), flush=True)

# the share of a test_conversion_f0(tracker="viterbi") batch: its stages on 64 clips of 10 s, the three tracker calls among them
model = models.VQVAE(1, 256, 512, n_speakers=4).to(dev).eval()
lens = np.full(B, L, dtype=np.int64)
mel = Au.melspectrogram(wav, lengths=lens)
Tc = mel.shape[2] // 4 * 4
g = torch.arange(B, dtype=torch.int64) % 4
angles = torch.rand(B, Tc, 513, device=dev, generator=torch.Generator(dev).manual_seed(0))
_, conv = evaluate.convert_voice(model, mel[:, :, :Tc].contiguous(), g)
wav_c = Au.inv_mel_spectrogram(conv.squeeze(1), angles0=angles)
frames, frames_c = np.full(B, mel.shape[2], dtype=np.int32), np.full(B, Tc, dtype=np.int32)
ft = track[2]


def three(fn):
    fn(wav_c)
    fn(wav, lengths=lens)
    fn(wav, lengths=lens)


def two_warpings():
    cep_t = Au.mel_cepstra(mel, frames)
    for m, fr in ((conv, frames_c), (mel, frames)):
        cost, steps, path = ops.dtw(Au.mel_cepstra(m, fr), cep_t, fr, frames, want_path=True)
        ops.f0_path_stats(ft[:, :m.shape[-1]].contiguous(), ft, path, steps)


t_mel, t_conv, t_inv, t_yin, t_trk, t_warp = (w[0] for w in windows([
    lambda: (Au.melspectrogram(wav, lengths=lens), Au.melspectrogram(wav, lengths=lens)),
    lambda: evaluate.convert_voice(model, mel[:, :, :Tc].contiguous(), g), lambda: Au.inv_mel_spectrogram(conv.squeeze(1), angles0=angles),
    lambda: three(Au.f0), lambda: three(Au.f0_track), two_warpings]))
rest = t_mel + t_conv + t_inv + t_warp
rec = dict(conversion_f0_batch=dict(clips=B, frames=int(mel.shape[2]), dim=256, codes=512, griffin_lim_iters=Au.GRIFFIN_LIM_ITERS),
           two_melspectrograms_ms=t_mel * 1e3, convert_voice_ms=t_conv * 1e3, inv_mel_spectrogram_ms=t_inv * 1e3, three_f0_ms=t_yin * 1e3,
           three_f0_track_ms=t_trk * 1e3, two_warpings_with_stats_ms=t_warp * 1e3, f0_share=t_yin / (rest + t_yin),
           f0_track_share=t_trk / (rest + t_trk))
results.append(rec)
print(json.dumps(rec), flush=True)
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results, fh, indent=1)
