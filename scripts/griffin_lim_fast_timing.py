"""Timing and convergence of fast Griffin-Lim (audio.griffin_lim(momentum=0.99) = nsg_audio_griffin_lim_fast) against the plain
iteration (momentum 0 = nsg_audio_griffin_lim, the kernels and launches there were), on 64 clips of 862 frames (10 s at 22 050 Hz),
n_fft 1024, hop 256: the magnitudes are mel_to_linear of a mel decoded by a randomly initialised speaker-conditioned VQ-VAE from
synthetic voiced clips (scripts/f0_timing.py's).  Every call is warmed up, then timed in windows of whole calls that end in a
device synchronise; the figure is the median window.  Reported: both at 60 iterations and per iteration (the 0-iteration call,
the initial phases and one istft, subtracted), the bytes an iteration moves before and after, the spectral convergence of each
at 8, 16, 30 and 60 iterations from the same initial phases, and the audio.spectral_convergence call alone (with the frames' sums,
and through the ABI without them: one workgroup per clip).  With --lib PATH, another build of libnsg.so (the parent commit's, built
in a checkout of its own) runs the plain 60 iterations alternately with this one, in this process, and the waveforms are compared.
There is no fallback: without a GPU this fails.    python scripts/griffin_lim_fast_timing.py [--json out.json] [--lib other/libnsg.so]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_sound_generation_amd import _lib, audio as Au, evaluate, models
from neural_sound_generation_amd.ops import _p, _stream

if not torch.cuda.is_available():
    raise SystemExit("griffin_lim_fast_timing: needs a GPU (cuda:0)")
dev = torch.device("cuda:0")
WINDOWS, MIN_WINDOW_S = 7, 0.25
SR, HOP, NFFT = 22050, 256, 1024
MOMENTUM = 0.99


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
wav = torch.from_numpy(np.stack([voiced_clip(L, b) for b in range(B)])).to(dev)
torch.manual_seed(0)
model = models.VQVAE(1, 256, 512, n_speakers=4).to(dev).eval()
mel = Au.melspectrogram(wav, lengths=np.full(B, L, dtype=np.int64))
T = mel.shape[2]                                       # 862: decoded frame by frame below, whatever T mod 4 is
Tc = T // 4 * 4
_, conv = evaluate.convert_voice(model, mel[:, :, :Tc].contiguous(), torch.arange(B, dtype=torch.int64) % 4)
decoded = torch.cat((conv.squeeze(1), conv.squeeze(1)[:, :, :T - Tc]), dim=2).contiguous()       # (B, 80, 862)
S = Au.mel_to_linear(decoded)
F = S.shape[2]
u = torch.rand(B, T, F, device=dev, generator=torch.Generator(dev).manual_seed(0))
assert tuple(S.shape) == (B, 862, 513)

# the convergence of both iterations from the same initial phases
conv_rows = []
for iters in (8, 16, 30, 60):
    row = dict(iterations=iters)
    for name, m in (("plain", 0.0), ("momentum_0.99", MOMENTUM)):
        sc = Au.spectral_convergence(Au.griffin_lim(S, NFFT, HOP, iters, u, momentum=m), S, NFFT, HOP)
        row[name] = dict(mean=float(sc.mean()), min=float(sc.min()), max=float(sc.max()))
    conv_rows.append(row)
    print(json.dumps(row), flush=True)
results.append(dict(spectral_convergence=conv_rows, clips=B, frames=T, n_fft=NFFT, hop=HOP))

# time: 60 iterations, and the 0-iteration call to subtract
state = torch.empty(B, T, F, dtype=torch.complex64, device=dev)
t0 = median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 0, u))
plain = median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 60, u))
fast = median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 60, u, momentum=MOMENTUM, state=state))
plain16 = median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 16, u))
fast16 = median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 16, u, momentum=MOMENTUM, state=state))
per_plain, per_fast = (plain[0] - t0[0]) / 60, (fast[0] - t0[0]) / 60
# bytes an iteration moves per frame, each array once: the phase kernel reads hop new samples and S and writes the spectrum; the
# istft reads the spectrum and writes the frame; the overlap-add reads the frames and writes hop samples.  Momentum: c read and written.
bytes_plain = 4 * HOP + F * (4 + 8) + F * 8 + 4 * NFFT + 4 * NFFT + 4 * HOP
bytes_fast = bytes_plain + F * 16
rec = dict(clips=B, frames=T, n_fft=NFFT, hop=HOP, windows=WINDOWS, zero_iterations_ms=t0[0] * 1e3,
           plain_60_ms=plain[0] * 1e3, plain_60_ms_min=plain[1] * 1e3, plain_60_ms_max=plain[2] * 1e3,
           momentum_60_ms=fast[0] * 1e3, momentum_60_ms_min=fast[1] * 1e3, momentum_60_ms_max=fast[2] * 1e3,
           plain_16_ms=plain16[0] * 1e3, momentum_16_ms=fast16[0] * 1e3,
           plain_per_iteration_us=per_plain * 1e6, momentum_per_iteration_us=per_fast * 1e6, momentum_over_plain=per_fast / per_plain,
           bytes_per_frame_plain=bytes_plain, bytes_per_frame_momentum=bytes_fast, bytes_ratio=bytes_fast / bytes_plain,
           plain_GBps=bytes_plain * B * T / per_plain / 1e9, momentum_GBps=bytes_fast * B * T / per_fast / 1e9)
results.append(rec)
print(json.dumps(rec), flush=True)

# against another build of the library (--lib PATH: the parent commit's libnsg.so, say): nsg_audio_griffin_lim x 60 through it and
# through this one, alternately in this process, three rounds; an older library need not export the new entry points
if "--lib" in sys.argv:
    import ctypes
    from neural_sound_generation_amd import ops
    other = ctypes.CDLL(os.path.abspath(sys.argv[sys.argv.index("--lib") + 1]))
    for name in ("nsg_audio_griffin_lim_workspace_bytes", "nsg_audio_griffin_lim"):
        getattr(other, name).restype, getattr(other, name).argtypes = _lib._SIGS[name]
    ws, nb = ops._ws(dev, "nsg_audio_griffin_lim_workspace_bytes", B, T, NFFT)
    assert other.nsg_audio_griffin_lim_workspace_bytes(B, T, NFFT) == nb
    y_other = torch.empty(B, HOP * (T - 1), device=dev)

    def plain_other():
        rc = other.nsg_audio_griffin_lim(_p(S), _p(u), _p(y_other), B, T, NFFT, HOP, 60, _p(ws), nb, _stream())
        assert rc == 0, rc

    plain_other()
    same_bits = bool(torch.equal(y_other, Au.griffin_lim(S, NFFT, HOP, 60, u)))
    rounds = []
    for _ in range(3):
        rounds.append(dict(other_ms=median_time(plain_other)[0] * 1e3, this_ms=median_time(lambda: Au.griffin_lim(S, NFFT, HOP, 60, u))[0] * 1e3))
    rec = dict(other_library=sys.argv[sys.argv.index("--lib") + 1], plain_60_rounds=rounds, same_bits=same_bits)
    results.append(rec)
    print(json.dumps(rec), flush=True)

# the figure's own cost
y = Au.griffin_lim(S, NFFT, HOP, 16, u, momentum=MOMENTUM)
clips = torch.empty(B, 2, dtype=torch.float64, device=dev)
t_sc = median_time(lambda: Au.spectral_convergence(y, S, NFFT, HOP))
t_serial = median_time(lambda: _lib.call("nsg_audio_spectral_convergence", _p(y), _p(S), _p(None), _p(clips), B, T, NFFT, HOP, _stream()))
rec = dict(spectral_convergence_ms=t_sc[0] * 1e3, spectral_convergence_ms_min=t_sc[1] * 1e3, spectral_convergence_ms_max=t_sc[2] * 1e3,
           without_frame_sums_ms=t_serial[0] * 1e3, share_of_one_plain_iteration=t_sc[0] / per_plain)
results.append(rec)
print(json.dumps(rec), flush=True)
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results, fh, indent=1)
