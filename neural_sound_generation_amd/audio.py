"""Mel -> waveform inversion, the audio export of the reference's epoch loop (src/main.py:164-197 calling
src/audio_tacotron.py:99-116): denormalise, dB -> amplitude, pseudo-inverse mel basis, power 1.5, Griffin-Lim (60
iterations), inverse pre-emphasis.  SURVEY.md section 8f row 4.

    inv_mel_spectrogram(mel_spectrogram, sample_rate, fft_size, hop_size, n_mel) -> waveform        (same signature)

An extension, opt-in (the defaults are the reference's): griffin_lim / inv_mel_spectrogram(momentum=m) is Griffin-Lim with momentum
("fast Griffin-Lim", Perraudin, Balazs, Sondergaard 2013: the phase of X + m (X - X_prev)), and spectral_convergence(y, S) reports
how far |stft(y)| still is from the magnitudes asked for, || |stft(y)| - S || / || S || per clip.

Another, opt-in too: spsi_phases(S) / inv_mel_spectrogram(init="spsi") starts Griffin-Lim from the phases of a single-pass
spectrogram inversion (Beauregard, Harish, Wyse 2015) instead of random ones: every spectral peak's phase advances by
hop (j + p) / n_fft turns a frame, j + p its parabola-refined bin, and the bins of its lobe are locked to it (include/nsg.h states
it; fp64 turns on the device, no FFT).  It buys the first iterations, not a better fixed point: on the export's mel magnitudes
the random start ends slightly lower at 60 iterations.

The arithmetic runs in libnsg.so (csrc/audio.hip: in-LDS FFT, fused STFT + phase update, overlap-add, recurrence); the mel
filterbank and its pseudo-inverse are constants built once on the host with numpy (librosa.filters.mel restated: Slaney
scale, area normalisation).  hparams are the reference's (src/hparams_tacotron.py:77-117: use_lws=False, power 1.5,
60 iterations, pre-emphasis 0.97, min_level_db -100, ref_level_db 20, fmin 125, fmax 7600, clipped [0, 1] normalisation).

The opposite direction, wav -> mel, is the reference's preprocessing (audio_tacotron.py:70-78 melspectrogram, :23-26 preemphasis):

    melspectrogram(wav, sample_rate, fft_size, hop_size, n_mels) -> (n_mels, T) normalised to [0, 1]  (same signature)

one kernel from samples to the normalised mel (pre-emphasis at the reflect-mapped index, Hann, FFT, |X| in LDS, the
filterbank as a band matrix, dB, normalise, clip; ragged batches, two layouts).

What the reference's multi-speaker preprocessing does to a recording before that (cmu_arctic.py:59-72):

    resample(wav, orig_sr, target_sr)    librosa.core.load(path, sr=22050)'s resampling (audio_tacotron.py:12-13)
    trim_silence(wav, top_db=20)         librosa.effects.trim(wav, top_db=20) -> (trimmed, (start, end))

resample is a band-limited Kaiser-windowed sinc interpolator in resampy's kaiser_best style, evaluated exactly per polyphase
phase from a table built in fp64 on the host (csrc/resample.hip; it makes no claim to reproduce resampy's table
interpolation); trim_silence restates librosa's frame energies and threshold.  read_wav reads PCM files with scipy at their
own rate; load_wav refuses a file at another rate unless resample=True, which sends it through the kernel.

Judging a converted utterance (evaluate.test_conversion): mel_cepstra (the DCT-II of each frame's log amplitude, coefficients
1 .. n_ceps), dtw (batched dynamic time warping, csrc/dtw.hip) and mel_cepstral_distortion, the two combined into the dB
figure of the voice-conversion literature.  An extension: the reference has no objective figure for converted speech.
Beside the envelope, the pitch (evaluate.test_conversion_f0): f0 (YIN on the waveform, csrc/f0.hip; frame t is mel frame t),
f0_distortion / f0_figures (F0 error in cents, voiced / unvoiced disagreement, log-F0 correlation along a dtw path);
f0_candidates / f0_track (opt-in: each frame's strongest local minima of YIN's d', and a min-sum path over them that chooses
one per frame or "unvoiced", csrc/f0_track.hip -- it repairs the octave errors and dropouts of a per-frame threshold).

Augmenting a recording (the reference's src/util.py:106-196: `sox tempo ... gain ...` per utterance and NoiseInjection; sox is
absent, so these are this project's definitions, include/nsg.h, not a parity claim): tempo (duration changed, pitch kept:
waveform-similarity overlap-add, csrc/tsm.hip), pitch_shift (tempo, then resample: pitch changed, duration kept), mix_noise (gain,
and a noise recording added at a level relative to the clip's RMS), random_augment (the reference's draws from a seeded CPU
generator, then tempo and mix_noise); preprocess.process_utterances(augment_copies=n) writes augmented copies.  All opt-in.

Judging a reconstruction against the recording it came from (evaluate.test_reconstruction_audio): stoi (STOI and, extended, ESTOI:
the short-time objective intelligibility of a processed waveform against the clean one, aligned sample for sample, at 10 kHz through
resample; csrc/stoi.hip), in two stages that can be called alone, stoi_envelopes and stoi_score; stoi_bands is the third-octave
table.  An extension: the reference has no figure in the waveform domain.  parity unpinned: pystoi is absent (here and on the GPU
box); the definition is this project's own, from the two papers, stated in include/nsg.h.

parity unpinned: librosa is absent (here, on the GPU box, and from the reference's own tree), and no file of the reference
holds a waveform; tests compare with the numpy restatement in oracle/audio_oracle.py (same initial phases) and check the
transform identities (istft(stft(y)) == y, the spectral error falls over the iterations).
"""
from __future__ import annotations

import functools
import math
from ctypes import c_void_p

import numpy as np
import torch

from . import _lib, ops
from .ops import _chk, _p, _stream, _ws

MIN_LEVEL_DB, REF_LEVEL_DB, MAX_ABS_VALUE = -100.0, 20.0, 1.0     # hparams_tacotron.py:99,110,111
POWER, GRIFFIN_LIM_ITERS, PREEMPHASIS = 1.5, 60, 0.97            # :116,117,107
FMIN, FMAX = 125.0, 7600.0                                        # :112,113


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


@functools.lru_cache(maxsize=8)
def mel_basis(sample_rate: int, fft_size: int, n_mels: int, fmin: float = FMIN, fmax: float = FMAX) -> np.ndarray:
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (audio_tacotron.py:208-219): (n_mels, 1 + fft_size/2) float32."""
    fftfreqs = np.linspace(0, sample_rate / 2.0, 1 + fft_size // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + fft_size // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


@functools.lru_cache(maxsize=8)
def _inv_mel_basis(sample_rate, fft_size, n_mels):
    return np.ascontiguousarray(np.linalg.pinv(mel_basis(sample_rate, fft_size, n_mels).astype(np.float64)).astype(np.float32))


def mel_to_linear(mel: torch.Tensor, sample_rate=22050, fft_size=1024, n_mels=80, power=POWER) -> torch.Tensor:
    """mel (B, n_mels, T) normalised to [0, 1] on the GPU -> Griffin-Lim's magnitudes S (B, T, 1 + fft_size/2)."""
    _chk(mel, "mel")
    B, M, T = mel.shape
    if M != n_mels:
        raise _lib.NsgError(f"mel_to_linear: expected {n_mels} mel bins, got {M}")
    F = fft_size // 2 + 1
    inv = torch.from_numpy(_inv_mel_basis(sample_rate, fft_size, n_mels)).to(mel.device)
    S = torch.empty(B, T, F, dtype=torch.float32, device=mel.device)
    _lib.call("nsg_audio_mel_to_linear", _p(mel), _p(inv), _p(S), B, M, T, F, MIN_LEVEL_DB, REF_LEVEL_DB, MAX_ABS_VALUE, power, _stream())
    return S


def _momentum(fn, momentum):
    """The momentum as the kernel gets it, rounded to fp32 (so a value that underflows to 0.f, 1e-50 say, is 0 here too and takes the
    plain iteration with every check that goes with it)."""
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float, np.integer, np.floating)) or not 0.0 <= momentum <= 1.0:
        raise ValueError(f"{fn}: momentum must be a number in [0, 1], got {momentum!r}")
    return float(np.float32(momentum))


def griffin_lim(S: torch.Tensor, fft_size=1024, hop_size=256, iters=GRIFFIN_LIM_ITERS, angles0: torch.Tensor | None = None, momentum=0.0,
                state: torch.Tensor | None = None) -> torch.Tensor:
    """S (B, T, F) magnitudes -> y (B, hop*(T-1)).  angles0: uniform [0,1) numbers for the initial phases (drawn if None).
    momentum in [0, 1]: 0 is the reference's iteration y <- istft(S X / |X|), X = stft(y); above 0 it is fast Griffin-Lim
    (Perraudin, Balazs, Sondergaard 2013; include/nsg.h: nsg_audio_griffin_lim_fast), which takes the phase of
    X + momentum (X - X_prev) instead and keeps one more spectrum (0.99 is librosa's default).  state: a complex64 (B, T, F) GPU
    tensor that receives X_iters, the last spectrum formed (momentum > 0 and iters >= 1; its content on entry is never read)."""
    _chk(S, "S")
    momentum = _momentum("griffin_lim", momentum)
    B, T, F = S.shape
    if F != fft_size // 2 + 1:
        raise _lib.NsgError(f"griffin_lim: S has {F} bins, fft_size {fft_size} needs {fft_size // 2 + 1}")
    if state is not None and (momentum == 0.0 or not torch.is_tensor(state) or state.dtype != torch.complex64 or tuple(state.shape) != (B, T, F)
                              or state.device != S.device or not state.is_contiguous()):
        raise ValueError(f"griffin_lim: state goes with momentum > 0 and is a contiguous complex64 tensor {(B, T, F)} on {S.device}")
    u = torch.rand(B, T, F, device=S.device) if angles0 is None else _chk(angles0.contiguous(), "angles0")
    y = torch.empty(B, hop_size * (T - 1), dtype=torch.float32, device=S.device)
    ws, nb = _ws(S.device, "nsg_audio_griffin_lim_workspace_bytes", B, T, fft_size)
    if momentum == 0.0:
        _lib.call("nsg_audio_griffin_lim", _p(S), _p(u), _p(y), B, T, fft_size, hop_size, iters, _p(ws), nb, _stream())
    else:
        c = torch.view_as_real(state) if state is not None else torch.empty(B, T, F, 2, dtype=torch.float32, device=S.device)
        _lib.call("nsg_audio_griffin_lim_fast", _p(S), _p(u), _p(y), _p(c), B, T, fft_size, hop_size, iters, momentum, _p(ws), nb, _stream())
    return y


def spsi_phases(S: torch.Tensor, fft_size=1024, hop_size=256) -> torch.Tensor:
    """Initial phases for griffin_lim by single-pass spectrogram inversion (Beauregard, Harish, Wyse 2015; include/nsg.h:
    nsg_audio_spsi_phases states the arithmetic): S (B, T, F) float32 magnitudes on the GPU -> (B, T, F) float32 on S's device, in
    turns in [0, 1), what griffin_lim takes as angles0.  Each spectral peak's phase advances by hop (j + p) / n_fft turns a frame, j + p
    its parabola-refined bin, and the bins around it are locked to it; fp64 on the device, a function of S alone bit for bit.
    fft_size in {512, 1024, 2048}, hop_size a divisor of it, T >= 1.  Every argument is checked before anything is launched."""
    if isinstance(fft_size, bool) or not isinstance(fft_size, (int, np.integer)) or fft_size not in (512, 1024, 2048):
        raise ValueError(f"spsi_phases: fft_size must be 512, 1024 or 2048, got {fft_size!r}")
    if isinstance(hop_size, bool) or not isinstance(hop_size, (int, np.integer)) or hop_size < 1 or fft_size % hop_size:
        raise ValueError(f"spsi_phases: hop_size must be a positive integer that divides fft_size = {fft_size}, got {hop_size!r}")
    if not torch.is_tensor(S) or S.dim() != 3 or S.shape[2] != fft_size // 2 + 1 or S.shape[0] < 1 or S.shape[1] < 1:
        raise ValueError(f"spsi_phases: expected magnitudes (B, T, {fft_size // 2 + 1}) with B, T >= 1 for fft_size {fft_size}, got "
                         f"{tuple(S.shape) if torch.is_tensor(S) else type(S).__name__}")
    _chk(S, "S")
    B, T, F = S.shape
    if B * T >= 2 ** 31:
        raise ValueError(f"spsi_phases: {B} clips of {T} frames are 2^31 frames or more")
    angles = torch.empty(B, T, F, dtype=torch.float32, device=S.device)
    ws, nb = _ws(S.device, "nsg_audio_griffin_lim_workspace_bytes", B, T, int(fft_size))
    _lib.call("nsg_audio_spsi_phases", _p(S), _p(angles), B, T, int(fft_size), int(hop_size), _p(ws), nb, _stream())
    return angles


INITS = ("random", "spsi")


def _init(fn, init, angles0):
    """inv_mel_spectrogram's `init` checked against its angles0, before anything is launched."""
    if not isinstance(init, str) or init not in INITS:
        raise ValueError(f"{fn}: init must be one of {INITS}, got {init!r}")
    if init == "spsi" and angles0 is not None:
        raise ValueError(f"{fn}: init='spsi' computes the initial phases itself; it does not go with angles0")
    return init


def spectral_convergence(y: torch.Tensor, S: torch.Tensor, fft_size=1024, hop_size=256, per_frame=False):
    """How far the waveforms y (B, hop*(T-1)) are from the magnitudes S (B, T, F) they were inverted from: the spectral
    convergence || |stft(y)| - S || / || S || per clip (Sturmel & Daudet 2011), on griffin_lim's grid, as a float64 (B,) tensor
    on the device: sqrt(num / den) of include/nsg.h's nsg_audio_spectral_convergence sums, 0 where both are 0 and inf where only
    den is 0.  per_frame=True also returns the (B, T, 2) sums {num, den} of every frame.  Nothing synchronises."""
    _chk(y, "y")
    _chk(S, "S")
    B, T, F = S.shape
    if F != fft_size // 2 + 1 or tuple(y.shape) != (B, hop_size * (T - 1)):
        raise _lib.NsgError(f"spectral_convergence: S {tuple(S.shape)} at fft_size {fft_size}, hop_size {hop_size} goes with y "
                            f"{(B, hop_size * (T - 1))} and {fft_size // 2 + 1} bins, got y {tuple(y.shape)}")
    frames = torch.empty(B, T, 2, dtype=torch.float64, device=S.device)
    clips = torch.empty(B, 2, dtype=torch.float64, device=S.device)
    _lib.call("nsg_audio_spectral_convergence", _p(y), _p(S), _p(frames), _p(clips), B, T, fft_size, hop_size, _stream())
    num, den = clips.unbind(1)
    sc = torch.where(num == 0, torch.zeros_like(num), torch.sqrt(num / den))
    return (sc, frames) if per_frame else sc


def stft(y: torch.Tensor, fft_size=1024, hop_size=256) -> torch.Tensor:
    """y (B, L) -> complex64 (B, 1 + L // hop, F): librosa.stft per row (frame-major)."""
    _chk(y, "y")
    B, L = y.shape
    X = torch.empty(B, 1 + L // hop_size, fft_size // 2 + 1, 2, dtype=torch.float32, device=y.device)
    _lib.call("nsg_audio_stft", _p(y), _p(X), B, L, fft_size, hop_size, _stream())
    return torch.view_as_complex(X)


@functools.lru_cache(maxsize=8)
def _mel_bands(sample_rate, fft_size, n_mels):
    """(n_mels, 2) int32: first and last non-zero bin of each filterbank row (first > last for an empty row).  Each Slaney
    triangle is non-zero on one contiguous run of bins; anything else is refused, since the kernel sums the run only."""
    basis = mel_basis(sample_rate, fft_size, n_mels)
    bands = np.empty((n_mels, 2), dtype=np.int32)
    for i in range(n_mels):
        nz = np.flatnonzero(basis[i])
        bands[i] = (nz[0], nz[-1]) if len(nz) else (1, 0)
        if len(nz) and len(nz) != nz[-1] - nz[0] + 1:
            raise ValueError(f"mel filter {i} of ({sample_rate}, {fft_size}, {n_mels}) is not one contiguous run of bins")
    return bands


@functools.lru_cache(maxsize=8)
def _mel_basis_on(sample_rate, fft_size, n_mels, device):
    return torch.from_numpy(mel_basis(sample_rate, fft_size, n_mels)).to(device)


def preemphasis(y: torch.Tensor, k=PREEMPHASIS) -> torch.Tensor:
    """audio_tacotron.py:23-26: p[n] = y[n] - k y[n-1], p[0] = y[0], per row of y (B, L)."""
    _chk(y, "y")
    B, L = y.shape
    out = torch.empty_like(y)
    _lib.call("nsg_audio_preemphasis", _p(y), _p(out), B, L, k, _stream())
    return out


LAYOUTS = {"mel_major": 0, "frame_major": 1}


def _on_device(wav, as_numpy, device):
    """The (B, L) float32 GPU batch the waveform kernels take: a numpy waveform uploaded to `device` as one clip, a tensor as it
    is -- on the GPU, float32 and contiguous, or an NsgError."""
    y = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)[None]).to(device) if as_numpy else wav
    return _chk(y, "wav")


def melspectrogram(wav, sample_rate=22050, fft_size=1024, hop_size=256, n_mels=80, lengths=None, layout="mel_major", device="cuda:0"):
    """audio_tacotron.py:70-78 with hparams_tacotron.py's settings.  wav: a 1-D numpy waveform as in the reference (returns a
    float32 numpy (n_mels, T), T = 1 + len // hop_size), or a float32 GPU tensor (B, L) of zero-padded clips (returns a GPU
    tensor).  lengths (B,) integers: clip b has lengths[b] samples, is reflect-padded at its own end, and its frames past
    1 + lengths[b] // hop_size are zeros; a clip's mel is bit for bit what it is alone.  layout: "mel_major" (B, n_mels, T),
    what VQVAE and mel_to_linear take, or "frame_major" (B, T, n_mels), the on-disk orientation.  Every argument is
    checked before anything is launched."""
    if layout not in LAYOUTS:
        raise ValueError(f"melspectrogram: layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    if fft_size not in (512, 1024, 2048) or hop_size <= 0 or n_mels <= 0:
        raise ValueError(f"melspectrogram: fft_size must be 512, 1024 or 2048 and hop_size, n_mels positive (got {fft_size}, {hop_size}, {n_mels})")
    as_numpy = isinstance(wav, np.ndarray)
    if as_numpy:
        if wav.ndim != 1 or not np.issubdtype(wav.dtype, np.floating):
            raise TypeError(f"melspectrogram: a numpy waveform must be 1-D floating point, got {wav.dtype} {wav.shape}")
        B, L = 1, len(wav)
    else:
        if not torch.is_tensor(wav) or wav.dim() != 2 or wav.dtype != torch.float32:
            raise TypeError("melspectrogram: expected a 1-D numpy waveform or a float32 tensor (B, L)")
        B, L = wav.shape
    if L <= fft_size // 2:
        raise ValueError(f"melspectrogram: {L} samples; reflect padding needs more than fft_size / 2 = {fft_size // 2}")
    lens = None
    if lengths is not None:
        host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"melspectrogram: lengths must be {B} integers, got {host.dtype} {host.shape}")
        if host.max() > L or host.min() <= fft_size // 2:
            raise ValueError(f"melspectrogram: every length must be in ({fft_size // 2}, {L}], got {int(host.min())} .. {int(host.max())}")
        lens = np.ascontiguousarray(host, dtype=np.int32)
    bands = _mel_bands(sample_rate, fft_size, n_mels)
    y = _on_device(wav, as_numpy, device)
    T = 1 + L // hop_size
    basis = _mel_basis_on(sample_rate, fft_size, n_mels, y.device)
    lens_d = torch.from_numpy(lens).to(y.device) if lens is not None else None
    out = torch.empty((B, T, n_mels) if LAYOUTS[layout] else (B, n_mels, T), dtype=torch.float32, device=y.device)
    _lib.call("nsg_audio_melspectrogram", _p(y), _p(lens_d), _p(basis), c_void_p(bands.ctypes.data), _p(out), B, L, fft_size, hop_size, n_mels,
              PREEMPHASIS, MIN_LEVEL_DB, REF_LEVEL_DB, MAX_ABS_VALUE, LAYOUTS[layout], _stream())
    return out[0].cpu().numpy() if as_numpy else out


@functools.lru_cache(maxsize=8)
def cepstra_table(n_mels: int, n_ceps: int, min_level_db: float = MIN_LEVEL_DB) -> np.ndarray:
    """(n_ceps, n_mels) float32: rows 1 .. n_ceps of the orthonormal DCT-II over the bands, scaled from the normalised mel to
    the natural-log amplitude (a normalised mel m is the level min_level_db * (1 - m) dB + constants, i.e. ln amplitude =
    m * (-min_level_db) * ln 10 / 20 + constants).  Row 0 (the energy) is left out, and with it every additive constant.
        table[k][j] = (-min_level_db ln 10 / 20) sqrt(2 / n_mels) cos(pi (k + 1) (j + 1/2) / n_mels)
    computed in fp64 and rounded once."""
    k = np.arange(1, n_ceps + 1, dtype=np.float64)[:, None]
    j = np.arange(n_mels, dtype=np.float64)[None, :]
    t = (-float(min_level_db) * math.log(10.0) / 20.0) * math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (j + 0.5) / n_mels)
    return np.ascontiguousarray(t.astype(np.float32))


@functools.lru_cache(maxsize=8)
def _cepstra_table_on(n_mels, n_ceps, min_level_db, device):
    return torch.from_numpy(cepstra_table(n_mels, n_ceps, min_level_db)).to(device)


def _mel3(mel, name):
    if torch.is_tensor(mel) and mel.dim() == 4 and mel.shape[1] == 1:
        mel = mel[:, 0]
    if not torch.is_tensor(mel) or mel.dim() != 3:
        raise ValueError(f"{name}: expected a mel tensor (B, n_mels, T) or (B, 1, n_mels, T)")
    return mel


def mel_cepstra(mel, frames=None, n_ceps=13, min_level_db=MIN_LEVEL_DB):
    """Normalised mels (B, n_mels, T) or (B, 1, n_mels, T) on the GPU -> their mel cepstra (B, T, n_ceps), frame-major:
    coefficients 1 .. n_ceps of the DCT-II of each frame's log amplitude (cepstra_table).  frames (B,): valid frames per clip;
    the coefficients of later frames are +0.0."""
    mel = _mel3(mel, "mel_cepstra")
    if not 1 <= int(n_ceps) < mel.shape[1]:
        raise ValueError(f"mel_cepstra: n_ceps = {n_ceps} outside [1, n_mels - 1 = {mel.shape[1] - 1}] (the DCT of n_mels bands has that many rows past the energy)")
    return ops.mel_cepstra(mel, _cepstra_table_on(mel.shape[1], int(n_ceps), float(min_level_db), mel.device), frames)


def dtw(a, b, len_a=None, len_b=None, want_path=False):
    """Dynamic time warping of feature sequences a (B, Ta, K), b (B, Tb, K) under the Euclidean frame distance, steps
    (1, 1), (1, 0), (0, 1) -> cost (B,), steps (B,) [, path (B, Ta + Tb - 1, 2)] (ops.dtw).  A length of None is the whole
    tensor's."""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.dim() != 3 or b.dim() != 3:
        raise ValueError("dtw: expected tensors a (B, Ta, K) and b (B, Tb, K)")
    B = a.shape[0]
    return ops.dtw(a, b, np.full(B, a.shape[1], dtype=np.int32) if len_a is None else len_a,
                   np.full(B, b.shape[1], dtype=np.int32) if len_b is None else len_b, want_path)


MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)       # nepers of cepstral distance -> dB


def mel_cepstral_distortion(mel_a, mel_b, frames_a=None, frames_b=None, n_ceps=13):
    """Mel-cepstral distortion of parallel clips after dynamic time warping: the Euclidean distance of the two frames' mel
    cepstra (coefficients 1 .. n_ceps), summed along the cheapest warping path and divided by its length, in dB:
        mcd = (10 sqrt(2) / ln 10) * cost / steps
    (the constant is applied once, to the quotient).  mel_a (B, n_mels, Ta), mel_b (B, n_mels, Tb) normalised mels (or
    (B, 1, n_mels, T)); frames_a, frames_b (B,) valid frames per clip, at least 1 (None: all).  Returns (mcd (B,) float32,
    steps (B,) int32) on the device; nothing here synchronises when the frame counts are given on the host."""
    mel_a, mel_b = _mel3(mel_a, "mel_cepstral_distortion"), _mel3(mel_b, "mel_cepstral_distortion")
    if mel_a.shape[0] != mel_b.shape[0] or mel_a.shape[1] != mel_b.shape[1]:
        raise ValueError(f"mel_cepstral_distortion: {tuple(mel_a.shape)} and {tuple(mel_b.shape)} are not parallel batches of one band count")
    B = mel_a.shape[0]
    fa = np.full(B, mel_a.shape[2], dtype=np.int32) if frames_a is None else frames_a
    fb = np.full(B, mel_b.shape[2], dtype=np.int32) if frames_b is None else frames_b
    fa = ops._lengths_on(fa, "mel_cepstral_distortion: frames_a", B, 1, mel_a.shape[2], mel_a.device)
    fb = ops._lengths_on(fb, "mel_cepstral_distortion: frames_b", B, 1, mel_b.shape[2], mel_b.device)
    cost, steps = ops.dtw(mel_cepstra(mel_a, fa, n_ceps), mel_cepstra(mel_b, fb, n_ceps), fa, fb)
    return (cost / steps.to(torch.float32)) * MCD_DB, steps


F0_MAX_LAG = 1024                     # include/nsg.h: the longest lag nsg_audio_f0 searches


def f0_lags(sample_rate, fmin, fmax):
    """(tau_min, tau_max) = (ceil(sample_rate / fmax), floor(sample_rate / fmin)): the lags, in samples, of the periods of
    [fmin, fmax].  ValueError unless 0 < fmin <= fmax and 1 <= tau_min <= tau_max <= F0_MAX_LAG."""
    if not (sample_rate > 0 and 0 < fmin <= fmax):
        raise ValueError(f"f0: need sample_rate > 0 and 0 < fmin <= fmax, got {sample_rate!r}, {fmin!r}, {fmax!r}")
    tau_min, tau_max = int(math.ceil(sample_rate / fmax)), int(math.floor(sample_rate / fmin))
    if not 1 <= tau_min <= tau_max <= F0_MAX_LAG:
        raise ValueError(f"f0: [{fmin}, {fmax}] Hz at {sample_rate} Hz are the lags [{tau_min}, {tau_max}]; need 1 <= tau_min <= tau_max <= {F0_MAX_LAG}")
    return tau_min, tau_max


def f0(wav, sample_rate=22050, hop_size=256, frame_length=1024, fmin=65.0, fmax=500.0, threshold=0.1, lengths=None, device="cuda:0"):
    """Fundamental frequency by YIN (de Cheveigne & Kawahara 2002; include/nsg.h states the arithmetic, csrc/f0.hip runs it): per
    frame t, centred on sample t * hop_size as mel frame t is, the cumulative-mean-normalised difference d' over the lags
    f0_lags(sample_rate, fmin, fmax) of a window of frame_length samples, the first lag with d' < threshold followed to its local
    minimum, refined by a parabola.  wav: a 1-D numpy waveform (returns numpy (f0 (T,), aperiodicity (T,)), T = 1 + len //
    hop_size), or a float32 GPU tensor (B, L) of zero-padded clips with optional lengths (B,) integers in [0, L] (returns GPU
    tensors (B, T)).  f0 is in Hz, +0.0 where a frame is unvoiced or past its clip's 1 + length // hop_size frames; aperiodicity
    is d' at the chosen lag (the least d' of an unvoiced frame, 1.0 past the clip).  The waveform is zero outside the clip; a
    clip's frames are bit for bit what they are alone.  With inv_mel_spectrogram's hop_size * (T - 1) samples this gives T
    frames: mel frame t and F0 frame t are the same instant.  Every argument is checked before anything is launched."""
    as_numpy, y, lens, tau_min, tau_max = _f0_args("f0", wav, sample_rate, hop_size, frame_length, fmin, fmax, lengths, device, threshold)
    freq, ap = ops.f0(y, int(frame_length), int(hop_size), tau_min, tau_max, float(threshold), float(sample_rate), lens)
    return (freq[0].cpu().numpy(), ap[0].cpu().numpy()) if as_numpy else (freq, ap)


def _f0_args(fn, wav, sample_rate, hop_size, frame_length, fmin, fmax, lengths, device, threshold=None):
    """The argument checks f0, f0_candidates and f0_track share (threshold: f0's alone), before anything is launched ->
    (as_numpy, the (B, L) GPU batch, int32 host lengths or None, tau_min, tau_max)."""
    if isinstance(frame_length, bool) or not isinstance(frame_length, (int, np.integer)) or frame_length % 2 or not 64 <= frame_length <= 2048:
        raise ValueError(f"{fn}: frame_length must be an even integer in [64, 2048], got {frame_length!r}")
    if isinstance(hop_size, bool) or not isinstance(hop_size, (int, np.integer)) or hop_size < 1:
        raise ValueError(f"{fn}: hop_size must be a positive integer, got {hop_size!r}")
    if threshold is not None and not 0 < threshold <= 1:
        raise ValueError(f"{fn}: threshold must be in (0, 1], got {threshold!r}")
    tau_min, tau_max = f0_lags(sample_rate, fmin, fmax)
    as_numpy, B, L, lens = _clip_batch(fn, wav, lengths, 0)
    if L < 1:
        raise ValueError(f"{fn}: an empty waveform")
    if B * (1 + L // hop_size) >= 2 ** 31:
        raise ValueError(f"{fn}: {B} clips of {1 + L // hop_size} frames are 2^31 frames or more")
    return as_numpy, _on_device(wav, as_numpy, device), lens, tau_min, tau_max


def f0_candidates(wav, sample_rate=22050, hop_size=256, frame_length=1024, fmin=65.0, fmax=500.0, lengths=None, device="cuda:0"):
    """The F0 candidates of every frame (include/nsg.h: nsg_audio_f0_candidates; csrc/f0.hip): the lags in f0_lags(sample_rate, fmin,
    fmax) at which YIN's d' has a local minimum below 1 -- of them the 8 with the least d', by ascending lag -- each refined by
    f0's parabola.  wav, lengths and the argument checks are f0's.  Returns (cand_f0 (T, 8) Hz, cand_ap (T, 8) = d' there, cand_logf
    (T, 8) = log2 cand_f0, count (T,) int32) as numpy for a numpy waveform, GPU tensors (B, T, 8) / (B, T) for a batch; slots past
    count hold (+0.0, 1.0, +0.0) and frames past a clip have count 0."""
    as_numpy, y, lens, tau_min, tau_max = _f0_args("f0_candidates", wav, sample_rate, hop_size, frame_length, fmin, fmax, lengths, device)
    out = ops.f0_candidates(y, int(frame_length), int(hop_size), tau_min, tau_max, float(sample_rate), lens)
    return tuple(t[0].cpu().numpy() for t in out) if as_numpy else out


# Praat's path-finder constants (Boersma 1993: octave cost, octave-jump cost, voiced / unvoiced cost) and, for the unvoiced state,
# the middle of the window 0.2 .. 0.45 in which the prototype signal (tests/test_f0_track_host.py) is tracked without an error
F0_TRACK_COSTS = dict(octave_cost=0.01, jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3)


def f0_track(wav, sample_rate=22050, hop_size=256, frame_length=1024, fmin=65.0, fmax=500.0, lengths=None, device="cuda:0", octave_cost=0.01,
             jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3, detail=False):
    """Fundamental frequency by a path finder over YIN candidates (Boersma 1993, RAPT; include/nsg.h: nsg_audio_f0_candidates, then
    nsg_f0_viterbi): instead of taking each frame's first lag under a threshold, keep the frame's 8 strongest local minima of d'
    and let a dynamic programme choose one per frame, or "unvoiced".  A candidate costs its d' plus octave_cost per octave below
    the top of the range (logf_top = log2(sample_rate / tau_min)); the unvoiced state costs unvoiced_cost; a step between two
    candidates costs jump_cost per octave of the jump, a step between voiced and unvoiced vuv_cost.  This repairs f0's octave-up
    picks and its dropouts where the period's d' sits just above the threshold.  wav, lengths and the argument checks are f0's;
    a clip of `length` samples has 1 + length // hop_size frames.  Returns (f0, ap) in f0's shapes and conventions (ap of an
    unvoiced frame: the least d' of its candidates, 1.0 if none), with detail=True (f0, ap, state, cost): state (T,) int32 is 0
    for unvoiced, k for candidate slot k - 1 and -1 past the clip, cost the path's total.
    The four defaults are Praat's path-finder constants and, for unvoiced_cost, a value from the window 0.2 .. 0.45 that tracks
    the prototype signal without an error: a design choice, not a measurement on speech.  The costs are per frame step: they were
    chosen at hop_size / sample_rate = 11.6 ms, and a caller who moves far from that should rescale jump_cost and vuv_cost
    (a longer step allows a larger jump).  Every argument is checked before anything is launched."""
    costs = dict(octave_cost=octave_cost, jump_cost=jump_cost, vuv_cost=vuv_cost, unvoiced_cost=unvoiced_cost)
    for name, v in costs.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= v < float("inf"):
            raise ValueError(f"f0_track: {name} must be a finite number >= 0, got {v!r}")
    as_numpy, y, lens, tau_min, tau_max = _f0_args("f0_track", wav, sample_rate, hop_size, frame_length, fmin, fmax, lengths, device)
    cf, ca, cl, cnt = ops.f0_candidates(y, int(frame_length), int(hop_size), tau_min, tau_max, float(sample_rate), lens)
    frames = None if lens is None else 1 + lens // int(hop_size)
    out = ops.f0_viterbi(cl, ca, cf, cnt, math.log2(float(sample_rate) / tau_min), *(float(v) for v in costs.values()), frames=frames)
    state, cost, freq, ap = (t[0] for t in out) if as_numpy else out
    res = (freq, ap, state, cost) if detail else (freq, ap)
    return tuple(t.cpu().numpy() for t in res) if as_numpy else res


def f0_figures(stats):
    """The three pitch figures from rows of nsg_f0_path_stats sums, stats (..., 10) fp64 -> (rmse_cents, vuv_error, corr) fp64 (...):
        rmse_cents = 1200 sqrt(sum (x - y)^2 / n_vv)            the log-F0 error in cents over the cells both clips voice
        vuv_error  = (n_a_only + n_b_only) / steps              the share of cells one clip voices and the other does not
        corr       = (n sxy - sx sy) / sqrt((n sxx - sx^2)(n syy - sy^2))        Pearson's r of log2 F0 over those cells, n = n_vv
    rmse_cents and corr are NaN where n_vv < 2.  Rows may be sums of rows (pooling clips).  Computed where stats lives; nothing
    synchronises."""
    steps, n, na, nb, sx, sy, sxx, syy, sxy, sdd = stats.unbind(-1)
    nan = torch.full_like(n, float("nan"))
    few = n < 2
    rmse = torch.where(few, nan, 1200.0 * torch.sqrt(sdd / n))
    corr = torch.where(few, nan, (n * sxy - sx * sy) / torch.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy)))
    return rmse, (na + nb) / steps, corr


def f0_distortion(f0_a, f0_b, path, steps):
    """How two F0 tracks differ along a warping path (what ops.dtw / dtw(..., want_path=True) returns for the clips' cepstra):
    f0_a (B, Ta), f0_b (B, Tb) fp32 GPU tensors (+0.0: unvoiced), path (B, Ta + Tb - 1, 2) int32, steps (B,) int32 ->
    (rmse_cents (B,), vuv_error (B,), corr (B,), stats (B, 10)) fp64 on the device: f0_figures of ops.f0_path_stats."""
    stats = ops.f0_path_stats(f0_a, f0_b, path, steps)
    return (*f0_figures(stats), stats)


def _f0_batch(fn, f0):
    if not isinstance(f0, torch.Tensor) or f0.dim() != 2 or f0.dtype != torch.float32 or f0.shape[0] < 1 or f0.shape[1] < 1:
        raise ValueError(f"{fn}: f0 must be a float32 tensor (B, T) with B, T >= 1, as f0 / f0_track return it for a batch")
    return f0.shape


def f0_bins(f0, frames=None, n_bins=32, fmin=65.0, fmax=500.0, affine=None, detail=False):
    """An F0 track at the mel frame rate as the F0-conditioned decoder takes it: one bin per latent column (include/nsg.h:
    nsg_f0_bins states the arithmetic, csrc/f0_cond.hip runs it).  f0 (B, T) fp32 GPU tensor in Hz, +0.0 where unvoiced (f0 /
    f0_track); frames: None (all T), or (B,) valid frame counts in [0, T].  Latent column w of the T // 4 covers frames 4w .. 4w + 3;
    with at least two of them voiced and inside the clip its value is the mean of their log2 F0 -- moved by affine (B, 3) fp32 rows
    (mu_src, ratio, mu_tgt) to mu_tgt + (l - mu_src) ratio when given (f0_affine) -- and its bin 1 + the index of the n_bins equal
    log-frequency steps of [fmin, fmax] it falls into (clamped to the ends); otherwise the column is unvoiced, bin 0.
    Returns bins (B, T // 4) int64; with detail=True (bins, logf (B, T // 4) fp32: the moved mean log2 F0, +0.0 where unvoiced).
    ValueError before anything is launched: fewer than 4 frames, n_bins < 1, not 0 < fmin < fmax."""
    B, T = _f0_batch("f0_bins", f0)
    if T < 4:
        raise ValueError(f"f0_bins: {T} frames hold no latent column (4 frames each)")
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or n_bins < 1:
        raise ValueError(f"f0_bins: n_bins must be a positive integer, got {n_bins!r}")
    if not 0 < fmin < fmax < float("inf"):
        raise ValueError(f"f0_bins: need 0 < fmin < fmax, got {fmin!r}, {fmax!r}")
    return ops.f0_bins(f0.contiguous(), T // 4, int(n_bins), float(fmin), float(fmax), frames=frames, affine=affine, want_logf=detail)


def logf0_sums(f0, frames=None):
    """The moments of a clip's voiced log-F0: f0 (B, T) fp32 (+0.0: unvoiced), frames None or (B,) valid frame counts (a device
    tensor, or host integers) -> (B, 3) fp64 on f0's device: (n_voiced, sum log2 f0, sum (log2 f0)^2) over the frames t <
    frames[b] with f0 > 0, logarithms and sums in fp64.  Rows add: pooled over clips they give a speaker's statistics
    (evaluate.speaker_f0_stats).  Nothing synchronises."""
    B, T = _f0_batch("logf0_sums", f0)
    voiced = f0 > 0
    if frames is not None:
        fr = frames if isinstance(frames, torch.Tensor) else torch.as_tensor(np.asarray(frames).astype(np.int64))
        if tuple(fr.shape) != (B,):
            raise ValueError(f"logf0_sums: frames must hold {B} counts, got {tuple(fr.shape)}")
        voiced = voiced & (torch.arange(T, device=f0.device).unsqueeze(0) < fr.to(f0.device).unsqueeze(1))
    l = torch.where(voiced, torch.log2(torch.where(voiced, f0, torch.ones_like(f0)).double()), torch.zeros((), dtype=torch.float64, device=f0.device))
    return torch.stack((voiced.sum(1).double(), l.sum(1), (l * l).sum(1)), dim=1)


F0_AFFINE_MIN_VAR = 1e-12             # octaves^2: below it a source's spread is the rounding of its moments' difference -- "zero"


def f0_affine(sums_src, target_mean, target_std):
    """The move of a source contour to a target speaker's log-F0 statistics, as f0_bins takes it: sums_src (B, 3) fp64 rows of
    logf0_sums (each source clip's own moments), target_mean and target_std (B,) (tensors, or numbers for all clips) in log2 Hz
    -> (B, 3) fp32 rows (mu_src, ratio, mu_tgt) on sums_src's device:
        mu_src = sum / n,  var_src = sumsq / n - mu_src^2,  ratio = target_std / sqrt(var_src),  mu_tgt = target_mean
    with ratio = 1 where the source has fewer than 2 voiced frames or zero spread (var_src <= F0_AFFINE_MIN_VAR), and mu_src =
    mu_tgt where it has no voiced frame (nothing moves: such a clip has no voiced column either).  fp64 until the final rounding;
    nothing synchronises."""
    if not isinstance(sums_src, torch.Tensor) or sums_src.dim() != 2 or sums_src.shape[1] != 3 or sums_src.dtype != torch.float64:
        raise ValueError("f0_affine: sums_src must be (B, 3) fp64 rows of logf0_sums")
    B, dev = sums_src.shape[0], sums_src.device
    mt, st = (torch.as_tensor(v, dtype=torch.float64, device=dev).expand(B) if not isinstance(v, torch.Tensor) or v.dim() == 0
              else v.to(device=dev, dtype=torch.float64) for v in (target_mean, target_std))
    if tuple(mt.shape) != (B,) or tuple(st.shape) != (B,):
        raise ValueError(f"f0_affine: target_mean and target_std must be numbers or hold {B} values")
    n, s1, s2 = sums_src.unbind(1)
    some = n > 0
    n1 = torch.where(some, n, torch.ones_like(n))
    mu = torch.where(some, s1 / n1, mt)
    var = torch.where(some, s2 / n1 - (s1 / n1) ** 2, torch.zeros_like(n))
    spread = (n >= 2) & (var > F0_AFFINE_MIN_VAR)
    ratio = torch.where(spread, st / torch.sqrt(torch.where(spread, var, torch.ones_like(var))), torch.ones_like(var))
    return torch.stack((mu, ratio, mt), dim=1).to(torch.float32).contiguous()


def inv_preemphasis(y: torch.Tensor, k=PREEMPHASIS) -> torch.Tensor:
    _chk(y, "y")
    B, L = y.shape
    out = torch.empty_like(y)
    _lib.call("nsg_audio_inv_preemphasis", _p(y), _p(out), B, L, k, _stream())
    return out


def inv_mel_spectrogram(mel_spectrogram, sample_rate=22050, fft_size=1024, hop_size=256, n_mel=80, iters=GRIFFIN_LIM_ITERS,
                        angles0=None, device="cuda:0", momentum=0.0, init="random"):
    """audio_tacotron.py:99-116.  mel_spectrogram: numpy (n_mel, T) as in the reference (returns a float32 numpy waveform), or a
    GPU tensor (B, n_mel, T) (returns a (B, hop*(T-1)) tensor).  momentum: griffin_lim's (0, the default, is the reference's).
    init: "random" (the default and the reference's: angles0, drawn if None) or "spsi": Griffin-Lim starts from
    spsi_phases(S) instead, which reaches a given spectral convergence in fewer iterations (not a better fixed point: DESIGN.md
    5k).  init="spsi" with an explicit angles0, or any other string, is a ValueError before anything is launched."""
    _init("inv_mel_spectrogram", init, angles0)
    as_numpy = isinstance(mel_spectrogram, np.ndarray)
    mel = torch.from_numpy(np.ascontiguousarray(mel_spectrogram, dtype=np.float32)).to(device) if as_numpy else mel_spectrogram
    y = _invert_mel(mel, sample_rate, fft_size, hop_size, n_mel, iters, angles0, momentum, init)[2]
    return y[0].cpu().numpy() if as_numpy else y


def _invert_mel(mel, sample_rate, fft_size, hop_size, n_mel, iters, angles0, momentum, init="random"):
    """inv_mel_spectrogram's steps on a GPU tensor -> (S, Griffin-Lim's waveform, the waveform after inverse pre-emphasis)."""
    _init("inv_mel_spectrogram", init, angles0)
    if mel.dim() == 2:
        mel = mel.unsqueeze(0)
    mel = mel.contiguous().float()
    S = mel_to_linear(mel, sample_rate, fft_size, n_mel)
    if angles0 is not None and not torch.is_tensor(angles0):
        angles0 = torch.from_numpy(np.ascontiguousarray(angles0, dtype=np.float32)).to(mel.device)
    if init == "spsi":
        angles0 = spsi_phases(S, fft_size, hop_size)
    y = griffin_lim(S, fft_size, hop_size, iters, angles0, momentum)
    return S, y, inv_preemphasis(y)


def save_wav(wav, path, sample_rate=22050):
    """audio_tacotron.py:15-18: peak-normalise to int16 and write."""
    from scipy.io import wavfile
    wav = np.asarray(wav, dtype=np.float32)
    wav = wav * (32767 / max(0.01, float(np.max(np.abs(wav)))))
    wavfile.write(path, sample_rate, wav.astype(np.int16))


def read_wav(path):
    """(sample rate, samples): the samples of a PCM file as float32 in [-1, 1) (int16 / int32 / uint8 scaled by their range,
    float as stored), the first channel of a multi-channel file, at the file's own rate."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim > 1:
        data = data[:, 0]
    if data.dtype == np.int16:
        return sr, data.astype(np.float32) / 32768.0
    if data.dtype == np.int32:
        return sr, (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    if data.dtype == np.uint8:
        return sr, (data.astype(np.float32) - 128.0) / 128.0
    if np.issubdtype(data.dtype, np.floating):
        return sr, np.ascontiguousarray(data, dtype=np.float32)
    raise ValueError(f"{path}: unsupported sample format {data.dtype}")


# The resampler's filter: Z zero crossings a side, roll-off and Kaiser beta.  These are resampy's kaiser_best parameters as
# recalled; resampy is not here to check them, so they are this project's constants, not a parity claim.
RESAMPLE_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA = 64, 0.9475937167399596, 14.769656459379492
RESAMPLE_MAX_TABLE = 1 << 20          # floats: ratios whose polyphase table is larger are refused


def resample_filter(u):
    """h(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u/Z)^2)) / I0(beta) for |u| < Z, else 0 (float64)."""
    u = np.asarray(u, dtype=np.float64)
    r2 = (u / RESAMPLE_ZEROS) ** 2
    inside = r2 < 1.0
    window = np.i0(RESAMPLE_BETA * np.sqrt(np.where(inside, 1.0 - r2, 0.0))) / np.i0(RESAMPLE_BETA)
    return np.where(inside, RESAMPLE_ROLLOFF * np.sinc(RESAMPLE_ROLLOFF * u) * window, 0.0)


def resample_ratio(orig_sr, target_sr):
    """(P, Q) = (target_sr, orig_sr) / gcd: P outputs for every Q inputs."""
    for nm, v in (("orig_sr", orig_sr), ("target_sr", target_sr)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError(f"resample: {nm} must be a positive integer, got {v!r}")
    g = math.gcd(int(orig_sr), int(target_sr))
    return int(target_sr) // g, int(orig_sr) // g


@functools.lru_cache(maxsize=16)
def resample_table(P: int, Q: int) -> np.ndarray:
    """The polyphase coefficients of the ratio P / Q, (P, 2W) float32, W = ceil(Z / s), s = min(1, P / Q): tap j of phase
    phi = (m Q) mod P multiplies x[floor(m Q / P) - W + 1 + j] by c[phi][j] = s h(s (phi / P + W - 1 - j)).  Evaluated in float64
    and rounded once.  16000 -> 22050 is 441 x 128; 48000 -> 22050 is 147 x 280."""
    if P <= 0 or Q <= 0 or math.gcd(P, Q) != 1:
        raise ValueError(f"resample_table: {P} / {Q} must be positive and in lowest terms")
    Z = RESAMPLE_ZEROS
    W = Z if P >= Q else -(-Z * Q // P)
    if P * 2 * W > RESAMPLE_MAX_TABLE:
        raise ValueError(f"resample: the ratio {P} / {Q} needs a table of {P} x {2 * W} = {P * 2 * W} coefficients, more than "
                         f"{RESAMPLE_MAX_TABLE}; resample in two steps or pick rates with a larger common divisor")
    s = min(1.0, P / Q)
    c = s * resample_filter(s * (np.arange(P)[:, None] / P + (W - 1 - np.arange(2 * W))[None, :]))
    c = c.astype(np.float32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=16)
def _resample_table_on(P, Q, device):
    """The kernel's layout of resample_table: tap-major, the phases in the order consecutive outputs meet them
    (column k = m mod P holds phase (k Q) mod P), so the lanes of a wave read consecutive floats."""
    c = resample_table(P, Q)
    return torch.from_numpy(np.ascontiguousarray(c[(np.arange(P) * Q) % P].T)).to(device)


def _clip_batch(fn, wav, lengths, shortest):
    """Shared argument checks of resample / trim_silence: (as_numpy, B, L, int32 host lengths or None)."""
    as_numpy = isinstance(wav, np.ndarray)
    if as_numpy:
        if wav.ndim != 1 or not np.issubdtype(wav.dtype, np.floating):
            raise TypeError(f"{fn}: a numpy waveform must be 1-D floating point, got {wav.dtype} {wav.shape}")
        if lengths is not None:
            raise ValueError(f"{fn}: lengths goes with a batch tensor, not with a numpy waveform")
        B, L = 1, len(wav)
    else:
        if not torch.is_tensor(wav) or wav.dim() != 2 or wav.dtype != torch.float32:
            raise TypeError(f"{fn}: expected a 1-D numpy waveform or a float32 tensor (B, L)")
        B, L = wav.shape
    if B < 1 or L < shortest:
        raise ValueError(f"{fn}: {B} clip(s) of {L} samples; need at least one clip of at least {shortest} samples")
    lens = None
    if lengths is not None:
        host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"{fn}: lengths must be {B} integers, got {host.dtype} {host.shape}")
        if host.max() > L or host.min() < shortest:
            raise ValueError(f"{fn}: every length must be in [{shortest}, {L}], got {int(host.min())} .. {int(host.max())}")
        lens = np.ascontiguousarray(host, dtype=np.int32)
    return as_numpy, B, L, lens


def resample(wav, orig_sr, target_sr, lengths=None, device="cuda:0"):
    """Band-limited resampling from orig_sr to target_sr, what librosa.core.load(path, sr=target_sr) does to a file at another
    rate (audio_tacotron.py:12-13), as a Kaiser-windowed sinc interpolator in resampy's kaiser_best style evaluated exactly per
    polyphase phase: with (P, Q) = resample_ratio(orig_sr, target_sr), s = min(1, P / Q) and h = resample_filter,

        y[m] = sum_n x[n] s h(s (m Q - n P) / P),   m < ceil(len P / Q),   x zero outside the clip.

    The last sample m = ceil(len P / Q) - 1 is evaluated like every other; librosa fixes the length to ceil too but would
    zero-pad that sample where resampy returned floor(len P / Q) of them.  wav: a 1-D numpy waveform (returns a float32
    numpy waveform), or a float32 GPU tensor (B, L) of zero-padded clips with optional lengths (B,) integers (returns
    (tensor (B, ceil(L P / Q)), out_lengths), out_lengths the int32 numpy array ceil(lengths P / Q); the rest of a row is
    zeros).  A clip's samples are bit for bit what they are alone.  orig_sr == target_sr returns the input unchanged.
    Every argument is checked before anything is launched."""
    P, Q = resample_ratio(orig_sr, target_sr)
    as_numpy, B, L, lens = _clip_batch("resample", wav, lengths, 1)
    if P == Q:
        return wav if as_numpy else (wav, lens if lens is not None else np.full(B, L, dtype=np.int32))
    W = resample_table(P, Q).shape[1] // 2
    L_out = -(-L * P // Q)
    if L_out >= 2 ** 31:
        raise ValueError(f"resample: {L} samples at {P} / {Q} give {L_out} samples, 2^31 or more")
    y = _on_device(wav, as_numpy, device)
    table =_resample_table_on(P, Q, str(y.device))
    lens_d = torch.from_numpy(lens).to(y.device) if lens is not None else None
    out = torch.empty(B, L_out, dtype=torch.float32, device=y.device)
    _lib.call("nsg_audio_resample", _p(y), _p(lens_d), _p(table), _p(out), B, L, P, Q, W, _stream())
    if as_numpy:
        return out[0].cpu().numpy()
    src = lens.astype(np.int64) if lens is not None else np.full(B, L, dtype=np.int64)
    return out, (-(-src * P // Q)).astype(np.int32)


_resample = resample          # load_wav's flag has the function's name


# The segment, search and overlap lengths of the tempo change, in milliseconds.  These are sox `tempo`'s defaults as recalled; sox
# is not here to check them, so they are this project's constants, not a parity claim.
TEMPO_SEGMENT_MS, TEMPO_SEARCH_MS, TEMPO_OVERLAP_MS = 82.0, 14.68, 12.0
TEMPO_RANGE, GAIN_RANGE_DB, NOISE_LEVELS = (0.85, 1.15), (-6.0, 8.0), (0.0, 0.5)      # util.py:122-123, :168


def tempo_sizes(sample_rate, segment_ms=TEMPO_SEGMENT_MS, search_ms=TEMPO_SEARCH_MS, overlap_ms=TEMPO_OVERLAP_MS):
    """(S, O, W) in samples: segment, overlap and search width, each round(sample_rate * ms / 1000); (1808, 265, 324) at 22 050 Hz.
    ValueError unless 1 <= O <= 2048, 2 O <= S <= 8192 and 1 <= W <= 2048 (include/nsg.h: nsg_audio_tempo's envelope)."""
    vals = []
    for nm, ms in (("segment_ms", segment_ms), ("overlap_ms", overlap_ms), ("search_ms", search_ms)):
        if isinstance(ms, bool) or not isinstance(ms, (int, float, np.integer, np.floating)) or not 0 < ms < float("inf"):
            raise ValueError(f"tempo: {nm} must be a positive finite number, got {ms!r}")
        vals.append(ms)
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float, np.integer, np.floating)) or not 0 < sample_rate < float("inf"):
        raise ValueError(f"tempo: sample_rate must be a positive finite number, got {sample_rate!r}")
    S, O, W = (int(round(float(sample_rate) * float(ms) / 1000.0)) for ms in vals)
    if not (1 <= O <= ops.TEMPO_MAX_OVERLAP and 2 * O <= S <= ops.TEMPO_MAX_SEGMENT and 1 <= W <= ops.TEMPO_MAX_SEARCH):
        raise ValueError(f"tempo: {segment_ms} / {overlap_ms} / {search_ms} ms at {sample_rate} Hz are S = {S}, O = {O}, W = {W} samples; need "
                         f"1 <= O <= {ops.TEMPO_MAX_OVERLAP}, 2 O <= S <= {ops.TEMPO_MAX_SEGMENT}, 1 <= W <= {ops.TEMPO_MAX_SEARCH}")
    return S, O, W


def _per_clip(fn, name, v, B, lo=None, hi=None, integer=False):
    """`v`, a number or B numbers, as a (B,) array (float64, or int64 with integer=True), checked to be finite and in [lo, hi]."""
    a = np.asarray(v)
    if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) if integer else np.issubdtype(a.dtype, np.number)) or np.iscomplexobj(a):
        raise ValueError(f"{fn}: {name} must be {'an integer' if integer else 'a number'} or {B} of them, got {v!r}")
    a = a.astype(np.int64 if integer else np.float64)
    a = np.broadcast_to(a, (B,)).copy() if a.ndim == 0 else a
    if a.shape != (B,) or not np.isfinite(a).all() or (lo is not None and a.min() < lo) or (hi is not None and a.max() > hi):
        raise ValueError(f"{fn}: {name} must be a finite number or {B} of them" + (f" in [{lo}, {hi}]" if lo is not None else "") + f", got {v!r}")
    return a


def tempo(wav, factor, sample_rate=22050, segment_ms=TEMPO_SEGMENT_MS, search_ms=TEMPO_SEARCH_MS, overlap_ms=TEMPO_OVERLAP_MS, lengths=None,
          device="cuda:0", detail=False):
    """Tempo change without pitch change, what `sox tempo <factor>` is for (util.py:106-119), by waveform-similarity overlap-add
    (include/nsg.h: nsg_audio_tempo states the arithmetic, csrc/tsm.hip runs it): the output is built from segments of S samples
    that overlap by O; segment m is taken from the input near m (S - O) factor, at the one of W positions where it continues the
    segment before it best (least sum of squared differences over the overlap), and cross-faded over the overlap.  (S, O, W) =
    tempo_sizes(sample_rate, segment_ms, search_ms, overlap_ms).  factor: a number or one per clip, in [0.25, 4]; above 1 is
    faster.  A clip of n samples gives floor(n / factor); factor 1 returns it bit for bit.  wav: a 1-D numpy waveform (returns
    a float32 numpy waveform), or a float32 GPU tensor (B, L) of zero-padded clips with optional lengths (B,) integers in [0, L]
    on the host (returns (tensor (B, max(1, max out_lengths)), out_lengths int32 numpy); the rest of a row is zeros).
    detail=True also returns positions, int32: the input sample each segment starts at ((M,) numpy, or (B, M_max) on the
    device with -1 past a clip's segments).  A clip's samples are bit for bit what they are alone.  Every argument is checked
    before anything is launched."""
    S, O, W = tempo_sizes(sample_rate, segment_ms, search_ms, overlap_ms)
    as_numpy, B, L, lens = _clip_batch("tempo", wav, lengths, 0)
    if L < 1:
        raise ValueError("tempo: an empty waveform")
    f = _per_clip("tempo", "factor", factor, B, ops.TEMPO_MIN_FACTOR, ops.TEMPO_MAX_FACTOR)
    res = ops.tempo(_on_device(wav, as_numpy, device), f, S, O, W, lens, want_positions=detail)
    if not as_numpy:
        return res
    n = int(res[1][0])
    out = res[0][0, :n].cpu().numpy()
    return (out, res[2][0, :-(-n // (S - O))].cpu().numpy()) if detail else out


def pitch_shift(wav, num, den, sample_rate=22050, lengths=None, device="cuda:0"):
    """Pitch times num / den with the duration kept: tempo(factor = den / num), which makes the clip num / den times as long at
    its own pitch, then resample(orig_sr = num, target_sr = den), the existing kernel, which plays that back den / num times as
    long: 196 / 185 is a semitone up.  num, den: positive integers with den / num in [0.25, 4] whose reduced ratio
    resample_table accepts (its refusal is let through).  A clip of n samples gives ceil(floor(n num / den) P / Q) samples, (P, Q)
    = resample_ratio(num, den) = (den, num) / gcd: n itself, or a sample or two off it.  wav and lengths as tempo takes them, every
    clip at least den / num samples long; returns a numpy waveform, or (tensor, out_lengths int32 numpy).  Every argument is
    checked before anything is launched."""
    P, Q = resample_ratio(num, den)
    if P != Q:
        resample_table(P, Q)
    as_numpy, B, L, lens = _clip_batch("pitch_shift", wav, lengths, 0)
    factor = float(den) / float(num)
    if not ops.TEMPO_MIN_FACTOR <= factor <= ops.TEMPO_MAX_FACTOR:
        raise ValueError(f"pitch_shift: den / num = {factor} outside [{ops.TEMPO_MIN_FACTOR}, {ops.TEMPO_MAX_FACTOR}]")
    src = lens if lens is not None else np.full(B, L, dtype=np.int32)
    if L < 1 or ops.tempo_out_lengths(src, factor).min() < 1:
        raise ValueError(f"pitch_shift: every clip must have at least den / num = {factor} samples")
    y, mid = tempo(_on_device(wav, as_numpy, device), factor, sample_rate, lengths=lens)
    out, out_lens = resample(y, int(num), int(den), lengths=mid)
    return out[0, :int(out_lens[0])].cpu().numpy() if as_numpy else (out, out_lens)


PSOLA_UNVOICED_S = 0.005             # the spacing of the marks on unvoiced stretches, in seconds
PSOLA_ALPHA = (1, 4)                 # a mark is looked for within a quarter period of where the period puts it
PSOLA_MIN_RATIO, PSOLA_MAX_RATIO = 0.5, 2.0


def psola_periods(sample_rate, fmin=65.0, fmax=500.0):
    """(P_u, P_min, P_max) in samples, as the PSOLA kernels take them: round(0.005 sample_rate), and f0_lags(sample_rate, fmin,
    fmax), the periods of [fmin, fmax]; (110, 45, 339) at 22 050 Hz.  ValueError unless 2 <= P_min <= P_max <= F0_MAX_LAG."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float, np.integer, np.floating)) or not 0 < sample_rate < float("inf"):
        raise ValueError(f"psola: sample_rate must be a positive finite number, got {sample_rate!r}")
    P_min, P_max = f0_lags(sample_rate, fmin, fmax)
    if P_min < 2:
        raise ValueError(f"psola: fmax = {fmax} Hz at {sample_rate} Hz is a period of {P_min} sample(s); need at least 2")
    return max(1, int(round(PSOLA_UNVOICED_S * float(sample_rate)))), P_min, P_max


def _psola_args(fn, wav, f0, sample_rate, hop_size, fmin, fmax, lengths, device):
    """The checks pitch_marks and pitch_shift_psola share, before anything is launched -> (as_numpy, B, the track as given, int32 host
    lengths or None, (P_u, P_min, P_max)); nothing is uploaded."""
    if isinstance(hop_size, bool) or not isinstance(hop_size, (int, np.integer)) or not ops.PSOLA_MIN_HOP <= hop_size <= ops.PSOLA_MAX_HOP:
        raise ValueError(f"{fn}: hop_size must be an integer in [{ops.PSOLA_MIN_HOP}, {ops.PSOLA_MAX_HOP}], got {hop_size!r}")
    periods = psola_periods(sample_rate, fmin, fmax)
    as_numpy, B, L, lens = _clip_batch(fn, wav, lengths, 0)
    if L < 1:
        raise ValueError(f"{fn}: an empty waveform")
    if B * L >= 2 ** 31 - 1:
        raise ValueError(f"{fn}: {B} clips of {L} samples are 2^31 samples or more")
    f = _psola_track(fn, "f0", f0, as_numpy, B, None)
    return as_numpy, B, f, lens, periods


def _psola_track(fn, name, f0, as_numpy, B, T):
    """An F0 track that goes with the waveform: (T,) floating-point numpy for a numpy waveform, a float32 tensor (B, T) for a batch."""
    if as_numpy:
        if not isinstance(f0, np.ndarray) or f0.ndim != 1 or len(f0) < 1 or not np.issubdtype(f0.dtype, np.floating):
            raise TypeError(f"{fn}: with a numpy waveform {name} must be a 1-D floating-point numpy track, not empty")
        if T is not None and len(f0) != T:
            raise ValueError(f"{fn}: {name} has {len(f0)} frames, f0 has {T}")
        return f0
    if not torch.is_tensor(f0) or f0.dim() != 2 or f0.dtype != torch.float32 or f0.shape[0] != B or f0.shape[1] < 1:
        raise TypeError(f"{fn}: with a batch {name} must be a float32 tensor ({B}, T) with T >= 1")
    if T is not None and f0.shape[1] != T:
        raise ValueError(f"{fn}: {name} has {f0.shape[1]} frames, f0 has {T}")
    return f0


def _track_on(f0, as_numpy, device):
    return torch.from_numpy(np.ascontiguousarray(f0, dtype=np.float32)[None]).to(device) if as_numpy else f0


def pitch_marks(wav, f0, sample_rate=22050, hop_size=256, lengths=None, device="cuda:0", fmin=65.0, fmax=500.0):
    """Pitch marks for PSOLA (include/nsg.h: nsg_audio_pitch_marks states the chain, csrc/psola.hip runs it): one mark per period
    on the waveform's local maxima where the track `f0` (Hz, frame t at sample t * hop_size, a value not > 0: unvoiced, as f0 /
    f0_track return it) is voiced -- each looked for within a quarter period of where the period at the mark before it puts it,
    the earliest of equal maxima -- and one every 5 ms where it is not.  Periods are clamped into f0_lags(sample_rate, fmin, fmax).
    wav: a 1-D numpy waveform with a 1-D numpy track (returns (marks (K,) int32 numpy, K)), or a float32 GPU tensor (B, L) of
    zero-padded clips with a float32 track (B, T) and optional lengths (returns (marks (B, K_max) int32 with -1 past a clip's
    marks, n_marks (B,) int32) on the device).  A clip's marks are bit for bit what they are alone.  Every argument is checked
    before anything is launched."""
    as_numpy, B, f, lens, (P_u, P_min, P_max) = _psola_args("pitch_marks", wav, f0, sample_rate, hop_size, fmin, fmax, lengths, device)
    y = _on_device(wav, as_numpy, device)
    if not as_numpy and f.device != y.device:
        raise ValueError(f"pitch_marks: f0 on {f.device}, the batch on {y.device}")
    marks, n = ops.pitch_marks(y, _track_on(f, as_numpy, y.device), int(hop_size), float(sample_rate), P_u, P_min, P_max, PSOLA_ALPHA, lens)
    if not as_numpy:
        return marks, n
    k = int(n[0])
    return marks[0, :k].cpu().numpy(), k


def pitch_shift_psola(wav, f0, ratio=None, target_f0=None, sample_rate=22050, hop_size=256, lengths=None, device="cuda:0", detail=False,
                      fmin=65.0, fmax=500.0):
    """Pitch change with the spectral envelope and the duration kept, by time-domain pitch-synchronous overlap-add (Moulines &
    Charpentier 1990; include/nsg.h: nsg_audio_pitch_marks and nsg_audio_psola state the arithmetic, csrc/psola.hip runs it).
    Two-sided windowed grains are cut around pitch_marks(wav, f0) and laid down again at marks whose spacing is the local spacing
    divided by the pitch ratio, each taking the grain of the nearest analysis mark: the pulses come more or less often, each
    pulse's shape -- the formants -- stays, and the length is the input's, sample for sample.  (pitch_shift, tempo then resample,
    moves the formants with the pitch.)  Exactly one of
        ratio      a number or one per clip in [0.5, 2]: the output's track is f0 * ratio (an fp32 product);
        target_f0  the track the output is to have, in f0's form; only frames both tracks voice are moved
    f0: the clip's own track (Hz, frame t at sample t * hop_size, not > 0: unvoiced).  wav: a 1-D numpy waveform with 1-D numpy
    tracks (returns a float32 numpy waveform), or a float32 GPU tensor (B, L) with float32 tracks (B, T) and optional lengths
    (returns a tensor (B, L), zeros past each length).  ratio = 1 returns the input, exactly outside the marks and within a few
    roundings between them.  detail=True also returns (marks, n_marks, syn, map, n_syn) as ops.pitch_marks and ops.psola return
    them (numpy, cut to their counts, for a numpy waveform).  Every argument is checked before anything is launched."""
    if (ratio is None) == (target_f0 is None):
        raise ValueError("pitch_shift_psola: give exactly one of ratio and target_f0")
    as_numpy, B, f, lens, (P_u, P_min, P_max) = _psola_args("pitch_shift_psola", wav, f0, sample_rate, hop_size, fmin, fmax, lengths, device)
    if ratio is not None:
        r = _per_clip("pitch_shift_psola", "ratio", ratio, B, PSOLA_MIN_RATIO, PSOLA_MAX_RATIO)
    else:
        tgt = _psola_track("pitch_shift_psola", "target_f0", target_f0, as_numpy, B, f.shape[-1])
    if not as_numpy and (f.device != wav.device or (ratio is None and tgt.device != wav.device)):
        raise ValueError(f"pitch_shift_psola: the tracks are not on the batch's device {wav.device}")
    y = _on_device(wav, as_numpy, device)
    f_d = _track_on(f, as_numpy, y.device)
    f_out = f_d * torch.from_numpy(r.astype(np.float32)).to(y.device)[:, None] if ratio is not None else _track_on(tgt, as_numpy, y.device)
    P = (int(hop_size), float(sample_rate), P_u, P_min, P_max, PSOLA_ALPHA, lens)
    marks, n_marks = ops.pitch_marks(y, f_d, *P)
    out, syn, mp, n_syn = ops.psola(y, f_d, f_out.contiguous(), marks, n_marks, *P)
    if not as_numpy:
        return (out, marks, n_marks, syn, mp, n_syn) if detail else out
    res = out[0].cpu().numpy()
    if not detail:
        return res
    k, j = int(n_marks[0]), int(n_syn[0])
    return res, marks[0, :k].cpu().numpy(), k, syn[0, :j].cpu().numpy(), mp[0, :j].cpu().numpy(), j


PITCH_PERTURB_SEMITONES = (-4.0, 4.0)


def pitch_draws(n, generator, semitones=PITCH_PERTURB_SEMITONES):
    """The pitch perturbation's parameters for n clips from a CPU torch.Generator: per clip, in clip order, one fp64 u in [0, 1)
    (torch.rand(1, dtype=float64, generator=generator)), semitones = low + (high - low) u, ratio = 2^(semitones / 12) -> dict of
    (n,) fp64 arrays semitones, ratio.  Equal generator states give equal draws.  The range must lie inside [-12, 12]."""
    if not isinstance(generator, torch.Generator) or generator.device.type != "cpu":
        raise TypeError("perturb_pitch: generator must be a CPU torch.Generator")
    lo, hi = _range("perturb_pitch", "semitones", semitones)
    if lo < -12.0 or hi > 12.0:
        raise ValueError(f"perturb_pitch: semitones {semitones!r} outside [-12, 12] (a pitch ratio in [0.5, 2])")
    st = np.empty(n)
    for i in range(n):
        st[i] = lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=generator))
    return dict(semitones=st, ratio=np.clip(2.0 ** (st / 12.0), PSOLA_MIN_RATIO, PSOLA_MAX_RATIO))


def perturb_pitch(wav, lengths, generator, semitones=PITCH_PERTURB_SEMITONES, tracker="yin", tracker_options=None, sample_rate=22050):
    """Information perturbation for an F0-conditioned model: each clip's pitch moved by a random number of semitones with its
    formants and its length kept, so that what an encoder sees no longer tells the pitch the decoder must produce.  wav (B, L)
    float32 GPU tensor, lengths (B,) integers on the host or None.  The clips' F0 is tracked with f0 (tracker="yin") or f0_track
    ("viterbi") under tracker_options (their keyword arguments: hop_size, frame_length, fmin, fmax, ...); the shifts are
    pitch_draws(B, generator, semitones): a CPU torch.Generator, one draw per clip in clip order, so equal seeds give equal batches;
    then pitch_shift_psola(wav, f0, ratio) -> (out (B, L), params: semitones, ratio (B,) fp64 numpy and f0, the tracked (B, T)
    tensor).  Every argument is checked before anything is launched; pitch_shift, random_augment and augment_draws are untouched."""
    as_numpy, B, L, lens = _clip_batch("perturb_pitch", wav, lengths, 0)
    if as_numpy:
        raise TypeError("perturb_pitch: expected a float32 tensor (B, L)")
    if tracker not in ("yin", "viterbi"):
        raise ValueError(f"perturb_pitch: tracker must be 'yin' or 'viterbi', got {tracker!r}")
    opts = dict(tracker_options or {})
    if not set(opts) <= {"hop_size", "frame_length", "fmin", "fmax", "threshold", "octave_cost", "jump_cost", "vuv_cost", "unvoiced_cost"}:
        raise ValueError(f"perturb_pitch: tracker_options {sorted(opts)} has a key the trackers do not take")
    hop, fmin, fmax = opts.get("hop_size", 256), opts.get("fmin", 65.0), opts.get("fmax", 500.0)
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not ops.PSOLA_MIN_HOP <= hop <= ops.PSOLA_MAX_HOP:
        raise ValueError(f"perturb_pitch: hop_size must be an integer in [{ops.PSOLA_MIN_HOP}, {ops.PSOLA_MAX_HOP}], got {hop!r}")
    psola_periods(sample_rate, fmin, fmax)
    if L < 1:
        raise ValueError("perturb_pitch: an empty waveform")
    state = generator.get_state() if isinstance(generator, torch.Generator) else None
    params = pitch_draws(B, generator, semitones)
    try:
        track = (f0 if tracker == "yin" else f0_track)(wav, sample_rate=sample_rate, lengths=lens, **opts)[0]
    except Exception:
        generator.set_state(state)                     # a refused call draws nothing
        raise
    out = pitch_shift_psola(wav, track, ratio=params["ratio"], sample_rate=sample_rate, hop_size=int(hop), lengths=lens, fmin=fmin, fmax=fmax)
    params["f0"] = track
    return out, params


def mix_noise(wav, noise, level, offset, gain_db=0.0, lengths=None, device="cuda:0"):
    """Gain, then a noise recording added at `level` relative to the clip's RMS: util.py:185-196 (NoiseInjection.inject_noise_sample)
    with sox's `gain` (util.py:112-113) applied in front (include/nsg.h: nsg_audio_mix_noise):
        out_i = gain x_i + level sqrt(E_x / E_n) v_i,   v_i = noise[(offset + i) mod len(noise)],   gain = (float)10^(gain_db / 20)
    E_x, E_n the energies of the clip and of the noise under it (the gain does not enter the level: it is relative to the clip as
    given).  noise: one recording, a 1-D numpy array or a 1-D float32 GPU tensor, read cyclically from `offset`.  level, gain_db:
    a number or one per clip; offset: an integer or one per clip, in [0, len(noise)).  wav: a 1-D numpy waveform (returns numpy),
    or a float32 GPU tensor (B, L) with optional lengths (B,) in [0, L] (returns a tensor (B, L), zeros past each length).  Every
    argument is checked before anything is launched."""
    as_numpy, B, L, lens = _clip_batch("mix_noise", wav, lengths, 0)
    if L < 1:
        raise ValueError("mix_noise: an empty waveform")
    if isinstance(noise, np.ndarray):
        if noise.ndim != 1 or len(noise) < 1 or not np.issubdtype(noise.dtype, np.floating):
            raise TypeError(f"mix_noise: a numpy noise recording must be 1-D floating point and not empty, got {noise.dtype} {noise.shape}")
    elif not torch.is_tensor(noise) or noise.dim() != 1 or noise.dtype != torch.float32 or noise.shape[0] < 1:
        raise TypeError("mix_noise: noise must be a 1-D numpy array or a 1-D float32 tensor, not empty")
    Ln = len(noise)
    lv = _per_clip("mix_noise", "level", level, B)
    off = _per_clip("mix_noise", "offset", offset, B, 0, Ln - 1, integer=True)
    gain = 10.0 ** (_per_clip("mix_noise", "gain_db", gain_db, B) / 20.0)
    if gain.max() > float(np.finfo(np.float32).max):
        raise ValueError(f"mix_noise: gain_db = {gain_db!r} is not a finite fp32 gain")
    y = _on_device(wav, as_numpy, device)
    v = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(y.device) if isinstance(noise, np.ndarray) else noise
    out = ops.mix_noise(y, v, gain, lv, off, lens)
    return out[0].cpu().numpy() if as_numpy else out


def _range(fn, name, r):
    if not (isinstance(r, (tuple, list)) and len(r) == 2 and all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in r)
            and np.isfinite(r[0]) and np.isfinite(r[1]) and r[0] <= r[1]):
        raise ValueError(f"{fn}: {name} must be (low, high), finite, low <= high, got {r!r}")
    return float(r[0]), float(r[1])


def augment_draws(n, generator, tempo_range=TEMPO_RANGE, gain_range=GAIN_RANGE_DB, noise_len=None, noise_levels=NOISE_LEVELS):
    """The reference's random augmentation parameters for n clips (util.py:128-131 tempo and gain, :182 the noise level, :188 where
    the noise starts), from a CPU torch.Generator.  Per clip, in clip order, one fp64 u in [0, 1) per value (torch.rand(1,
    dtype=float64, generator=generator)) in this order: tempo = low + (high - low) u; gain_db likewise; and, when noise_len is
    given, level likewise and offset = min(floor(u noise_len), noise_len - 1).  -> dict of (n,) arrays: tempo, gain_db fp64, and
    level fp64, offset int64 with noise.  Equal generator states give equal draws."""
    if not isinstance(generator, torch.Generator) or generator.device.type != "cpu":
        raise TypeError("augment: generator must be a CPU torch.Generator")
    (t0, t1), (g0, g1), (l0, l1) = _range("augment", "tempo_range", tempo_range), _range("augment", "gain_range", gain_range), _range("augment", "noise_levels", noise_levels)
    if not ops.TEMPO_MIN_FACTOR <= t0 <= t1 <= ops.TEMPO_MAX_FACTOR:
        raise ValueError(f"augment: tempo_range {tempo_range!r} outside [{ops.TEMPO_MIN_FACTOR}, {ops.TEMPO_MAX_FACTOR}]")
    if noise_len is not None and noise_len < 1:
        raise ValueError("augment: an empty noise recording")

    def u():
        return float(torch.rand(1, dtype=torch.float64, generator=generator))

    p = dict(tempo=np.empty(n), gain_db=np.empty(n))
    if noise_len is not None:
        p.update(level=np.empty(n), offset=np.empty(n, dtype=np.int64))
    for i in range(n):
        p["tempo"][i] = t0 + (t1 - t0) * u()
        p["gain_db"][i] = g0 + (g1 - g0) * u()
        if noise_len is not None:
            p["level"][i] = l0 + (l1 - l0) * u()
            p["offset"][i] = min(int(u() * noise_len), noise_len - 1)
    return p


def random_augment(wav, lengths, generator, tempo_range=TEMPO_RANGE, gain_range=GAIN_RANGE_DB, noise=None, noise_levels=NOISE_LEVELS,
                   sample_rate=22050):
    """util.py:122-134 (load_randomly_augmented_audio) and, with `noise`, :180-196 (NoiseInjection.inject_noise) for a batch: each clip
    gets a tempo from tempo_range and a gain in dB from gain_range and, when noise (a 1-D recording, numpy or a float32 GPU tensor)
    is given, that recording from a random offset at a level from noise_levels relative to the clip's RMS.  The values are
    augment_draws(B, generator, ...): a CPU torch.Generator, a fixed order per clip (tempo, gain, level, offset), so equal seeds
    give equal batches.  wav (B, L) float32 GPU tensor, lengths (B,) integers on the host or None.  Runs tempo, then mix_noise
    (without noise: the gain alone) -> (out (B, max out_lengths), out_lengths int32 numpy, params: the draws)."""
    as_numpy, B, L, lens = _clip_batch("random_augment", wav, lengths, 0)
    if as_numpy:
        raise TypeError("random_augment: expected a float32 tensor (B, L)")
    Ln = None if noise is None else len(noise)
    params = augment_draws(B, generator, tempo_range, gain_range, Ln, noise_levels)
    y, out_lens = tempo(wav, params["tempo"], sample_rate, lengths=lens)
    if noise is None:
        out = mix_noise(y, torch.zeros(1, dtype=torch.float32, device=y.device), 0.0, 0, params["gain_db"], lengths=out_lens)
    else:
        out = mix_noise(y, noise, params["level"], params["offset"], params["gain_db"], lengths=out_lens)
    return out, out_lens, params


def trim_silence(wav, top_db=20.0, frame_length=2048, hop_length=512, lengths=None, device="cuda:0"):
    """librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) (cmu_arctic.py:72 calls it with top_db=20): the
    mean square of centred, reflect-padded frames, the loudest frame as the reference, and the span from the first to the last
    frame less than top_db below it: start = first * hop_length, end = min(len, (last + 1) * hop_length).  wav: a 1-D numpy
    waveform (returns (wav[start:end], (start, end)) as librosa does), or a float32 GPU tensor (B, L) of zero-padded clips
    with optional lengths (returns an int32 (B, 2) GPU tensor of (start, end); a clip's bounds do not depend on the batch).
    frame_length even in [2, 8192], hop_length >= 1, top_db > 0, every clip longer than frame_length / 2.  Every argument is
    checked before anything is launched."""
    if isinstance(frame_length, bool) or not isinstance(frame_length, (int, np.integer)) or frame_length % 2 or not 2 <= frame_length <= 8192:
        raise ValueError(f"trim_silence: frame_length must be an even integer in [2, 8192], got {frame_length!r}")
    if isinstance(hop_length, bool) or not isinstance(hop_length, (int, np.integer)) or hop_length < 1:
        raise ValueError(f"trim_silence: hop_length must be a positive integer, got {hop_length!r}")
    if not top_db > 0:
        raise ValueError(f"trim_silence: top_db must be positive, got {top_db!r}")
    as_numpy, B, L, lens = _clip_batch("trim_silence", wav, lengths, frame_length // 2 + 1)
    y = _on_device(wav, as_numpy, device)
    lens_d = torch.from_numpy(lens).to(y.device) if lens is not None else None
    bounds =torch.empty(B, 2, dtype=torch.int32, device=y.device)
    ws, nb = _ws(y.device, "nsg_audio_trim_workspace_bytes", B, L, hop_length)
    _lib.call("nsg_audio_trim_bounds", _p(y), _p(lens_d), _p(bounds), B, L, frame_length, hop_length, top_db, _p(ws), nb, _stream())
    if not as_numpy:
        return bounds
    start, end = (int(v) for v in bounds[0].cpu().numpy())
    return wav[start:end], (start, end)


def load_wav(path, sample_rate=22050, resample=False, device="cuda:0") -> np.ndarray:
    """audio_tacotron.py:12-13: the samples of a PCM file (read_wav) at sample_rate.  The reference resamples a file at another
    rate through librosa; here that is an error unless resample=True, which resamples it with `resample` on `device`."""
    sr, wav = read_wav(path)
    if sr != sample_rate:
        if not resample:
            raise ValueError(f"{path}: sample rate {sr}, expected {sample_rate} (pass resample=True to resample it)")
        wav = _resample(wav, sr, sample_rate, device=device)
    return wav


STOI_RATE, STOI_FRAME, STOI_HOP, STOI_FFT, STOI_BANDS, STOI_SEGMENT = 10000, 256, 128, 512, 15, 30     # include/nsg.h: nsg_audio_stoi_envelopes


@functools.lru_cache(maxsize=1)
def stoi_bands() -> np.ndarray:
    """The 15 third-octave bands of STOI as runs of the 512-point spectrum's bins at 10 kHz, (15, 2) int32 rows [lo, hi): with
    f[i] = i 10000 / 512, lo_j = argmin_i |f[i] - 150 * 2^((2 j - 1) / 6)| and hi_j = argmin_i |f[i] - 150 * 2^((2 j + 1) / 6)| (centre
    frequencies 150 * 2^(j / 3) Hz).  Band 0 is bins 7 .. 8, and hi_j = lo_{j+1}."""
    f = np.arange(STOI_FFT // 2 + 1, dtype=np.float64) * STOI_RATE / STOI_FFT
    j = np.arange(STOI_BANDS, dtype=np.float64)
    lo = np.argmin(np.abs(f[None, :] - (150.0 * 2.0 ** ((2.0 * j - 1.0) / 6.0))[:, None]), axis=1)
    hi = np.argmin(np.abs(f[None, :] - (150.0 * 2.0 ** ((2.0 * j + 1.0) / 6.0))[:, None]), axis=1)
    bands = np.ascontiguousarray(np.stack((lo, hi), axis=1), dtype=np.int32)
    bands.setflags(write=False)
    return bands


def _stoi_pair(fn, x, y, lengths):
    """The checks stoi_envelopes and stoi share, before anything is launched -> (B, L, host lengths or the device tensor or None)."""
    for nm, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise TypeError(f"{fn}: {nm} must be a float32 tensor (B, L), got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"{fn}: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} are not one aligned batch")
    B, L = x.shape
    if B < 1:
        raise ValueError(f"{fn}: an empty batch")
    if lengths is not None and not (torch.is_tensor(lengths) and lengths.is_cuda):
        host = lengths.numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"{fn}: lengths must be {B} integers, got {host.dtype} {host.shape}")
        if host.min() < 0 or host.max() > L:
            raise ValueError(f"{fn}: every length must be in [0, {L}], got {int(host.min())} .. {int(host.max())}")
        lengths = np.ascontiguousarray(host, dtype=np.int32)
    return B, L, lengths


def stoi_envelopes(x, y, lengths=None):
    """The first stage of stoi, at 10 kHz (include/nsg.h: nsg_audio_stoi_envelopes states it; csrc/stoi.hip): x the clean clips, y the
    processed ones, float32 GPU tensors (B, L) aligned sample for sample, L >= 256; lengths (B,) integers in [0, L] on the host, or
    an int32 tensor on the device (None: all L).  Frames of 256 samples every 128 under a Hann window; those whose energy in x is
    within 40 dB of the clip's loudest are kept, the kept frames of both signals are overlap-added into compacted signals, and
    those are analysed again (512-point FFT, 15 third-octave bands).  Returns (env (2, B, Tmax, 15) float32: the band envelopes
    of x and of y, zeros past each clip's kept frames; kept (B,) int32; src (B, Tmax) int32: the candidate frame behind each kept
    one, -1 beyond; energy (B, Tmax) float64: the candidates' energies), Tmax = (L - 256) // 128 + 1.  A clip shorter than 256
    samples keeps nothing.  A clip's outputs are bit for bit what they are alone.  parity unpinned: pystoi is absent, the
    definition is this project's, from the papers.  Every argument is checked before anything is launched; nothing synchronises."""
    B, L, lens = _stoi_pair("stoi_envelopes", x, y, lengths)
    if L < STOI_FRAME:
        raise ValueError(f"stoi_envelopes: {L} samples; a frame needs {STOI_FRAME}")
    Tmax = (L - STOI_FRAME) // STOI_HOP + 1
    if B * Tmax >= 2 ** 31:
        raise ValueError(f"stoi_envelopes: {B} clips of {Tmax} frames are 2^31 frames or more")
    _chk(x, "x")
    _chk(y, "y")
    lens_d = None if lens is None else ops._lengths_on(lens, "stoi_envelopes: lengths", B, 0, L, x.device)
    bands = stoi_bands()
    lo, hi = np.ascontiguousarray(bands[:, 0]), np.ascontiguousarray(bands[:, 1])
    energy = torch.empty(B, Tmax, dtype=torch.float64, device=x.device)
    src = torch.empty(B, Tmax, dtype=torch.int32, device=x.device)
    kept = torch.empty(B, dtype=torch.int32, device=x.device)
    env = torch.empty(2, B, Tmax, STOI_BANDS, dtype=torch.float32, device=x.device)
    _lib.call("nsg_audio_stoi_envelopes", _p(x), _p(y), _p(lens_d), c_void_p(lo.ctypes.data), c_void_p(hi.ctypes.data), _p(energy), _p(src), _p(kept),
              _p(env), B, L, _stream())
    return env, kept, src, energy


def stoi_score(env, kept, extended=False):
    """The second stage of stoi (include/nsg.h: nsg_audio_stoi_score): env (2, B, Tmax, 15) float32 and kept (B,) int32 as
    stoi_envelopes returns them -> d (B,) float64 on the device, NaN where kept < 30.  fp64 throughout."""
    if not isinstance(extended, (bool, np.bool_)):
        raise ValueError(f"stoi_score: extended must be a bool, got {extended!r}")
    if not torch.is_tensor(env) or env.dim() != 4 or env.shape[0] != 2 or env.shape[3] != STOI_BANDS or env.shape[1] < 1 or env.shape[2] < 1:
        raise ValueError(f"stoi_score: env must be (2, B, Tmax, {STOI_BANDS}) with B, Tmax >= 1")
    _, B, Tmax, _ = env.shape
    if not torch.is_tensor(kept) or tuple(kept.shape) != (B,) or kept.device != env.device:
        raise ValueError(f"stoi_score: kept must be an int32 tensor ({B},) on env's device")
    if B * Tmax >= 2 ** 31:
        raise ValueError(f"stoi_score: {B} clips of {Tmax} frames are 2^31 frames or more")
    _chk(env, "env")
    _chk(kept, "kept", torch.int32)
    d = torch.empty(B, dtype=torch.float64, device=env.device)
    _lib.call("nsg_audio_stoi_score", _p(env), _p(kept), _p(d), B, Tmax, int(bool(extended)), _stream())
    return d


def stoi(x, y, sample_rate=22050, lengths=None, extended=False):
    """Short-time objective intelligibility of processed clips y against the clean clips x (STOI: Taal, Hendriks, Heusdens, Jensen
    2011; extended=True: ESTOI, Jensen and Taal 2016), the waveform-domain figure for a reconstruction against its recording:
    insensitive to level and phase, it needs only a time-aligned pair.  x, y: float32 GPU tensors (B, L) at sample_rate, aligned
    sample for sample; lengths (B,) integers on the host (None: all L).  With sample_rate != 10000 both go through
    resample(., sample_rate, 10000, lengths) first (22 050 -> 10 000 is 200 / 441, a table of 200 x 284); at 10 000 lengths may
    also be an int32 device tensor.  Then stoi_envelopes and stoi_score (include/nsg.h states both): the correlation of the two
    signals' third-octave band envelopes over segments of 30 frames (384 ms), after the frames more than 40 dB below the clean
    clip's loudest are removed -- per band with the processed envelope scaled and clipped (STOI), or per segment after row and
    column normalisation (ESTOI).  Returns (d (B,) float64 on the device: about 1 for y = x, lower for worse, NaN where fewer
    than 30 frames are kept; kept (B,) int32 on the device).  parity unpinned: pystoi is absent (here and on the GPU box); the
    definition is this project's own, from the two papers, and tests compare with its numpy restatement.  Every argument is
    checked before anything is launched; nothing synchronises."""
    if not isinstance(extended, (bool, np.bool_)):
        raise ValueError(f"stoi: extended must be a bool, got {extended!r}")
    P, Q = resample_ratio(sample_rate, STOI_RATE)
    B, L, lens = _stoi_pair("stoi", x, y, lengths)
    if -(-L * P // Q) < STOI_FRAME:
        raise ValueError(f"stoi: {L} samples at {sample_rate} Hz are {-(-L * P // Q)} at {STOI_RATE} Hz; a frame needs {STOI_FRAME}")
    if P != Q:
        if lens is not None and not isinstance(lens, np.ndarray):
            raise ValueError("stoi: lengths on the device go with sample_rate = 10000 (the resampler takes them on the host)")
        if lens is not None and lens.min() < 1:
            raise ValueError(f"stoi: every length must be in [1, {L}] to be resampled, got {int(lens.min())}")
        resample_table(P, Q)
        x, lens10 = resample(x, sample_rate, STOI_RATE, lengths=lens)
        y, _ = resample(y, sample_rate, STOI_RATE, lengths=lens)
        lens = None if lens is None else lens10
    env, kept, _, _ = stoi_envelopes(x, y, lens)
    return stoi_score(env, kept, extended), kept
