"""CPU: the host side of the tempo / pitch / noise augmentation -- the restatements the GPU tests hold the kernels to
(tests/helpers/tempo_ref.py) on signals whose answer is known: the two exact consequences of writing the cross-fade as
a + w (b - a) (factor 1 is the identity, a periodic integer signal comes out as its own continuation), a tone whose pitch must
stay and, after the resampler, must move by num / den; the sizes; the header's declarations, their binding and their refusals;
the argument checks that raise before any kernel runs; the random draws."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, ops
from tests.helpers import resample64 as R64
from tests.helpers import tempo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 22050
F_TONE = 140.3


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def tone(seconds=2.0, freq=F_TONE, harmonics=6, sr=SR):
    n = np.arange(int(seconds * sr), dtype=np.float64)
    return sum(0.6 ** h * np.sin(2 * np.pi * freq * h * n / sr) for h in range(1, harmonics + 1)).astype(np.float32)


def peak_hz(y, start, window, sr=SR, lo=100.0, hi=260.0):
    """The spectral peak in [lo, hi] Hz of a Hann window of `window` samples from `start`, zero-padded to 2^18."""
    nfft = 1 << 18
    sp = np.abs(np.fft.rfft(np.asarray(y[start:start + window], dtype=np.float64) * np.hanning(window), nfft))
    a, b = int(lo * nfft / sr), int(hi * nfft / sr)
    return (a + int(np.argmax(sp[a:b]))) * sr / nfft


@pytest.fixture(scope="module")
def stretched():
    x = tone()
    return x, {f: R.wsola_f32(x, None, f) for f in (0.85, 1.15)}


def test_factor_one_is_the_identity():
    x = np.random.RandomState(0).standard_normal(5000).astype(np.float32)
    out, n, q = R.wsola_f32(x, None, 1.0, 64, 8, 20)
    assert n == 5000 and np.array_equal(bits(out), bits(x))
    assert np.array_equal(q, np.arange(len(q)) * 56)


@pytest.mark.parametrize("factor", [0.8, 0.85, 1.15, 1.25])
def test_a_periodic_integer_signal_is_continued_exactly(factor):
    period = np.random.RandomState(1).randint(-8, 9, 37).astype(np.float32)
    x = np.tile(period, 200)[:6000]
    out, n, q = R.wsola_f32(x, None, factor, 128, 16, 48)
    assert n == R.out_length(6000, factor)
    want = np.tile(period, 400)[:n]
    assert np.array_equal(bits(out[:n - 200]), bits(want[:n - 200]))
    m = np.flatnonzero(q + 128 + 48 <= 6000)                       # segments that read inside the clip: each one is in phase
    assert len(m) > 30 and (q[m] % 37 == (m * 112) % 37).all()


@pytest.mark.parametrize("factor,length", [(0.85, 51882), (1.15, 38347)])
def test_a_tone_keeps_its_pitch(stretched, factor, length):
    x, got = stretched
    out, n, q = got[factor]
    assert n == length == len(out) == int(np.floor(len(x) / factor))
    f = peak_hz(out, 8192, 16384)
    print(f"factor {factor}: peak {f:.3f} Hz")
    assert abs(f - F_TONE) < 0.25
    o64, n64, q64 = R.wsola_f64(x, None, factor)
    assert n64 == n and abs(peak_hz(o64, 8192, 16384) - F_TONE) < 0.25


@pytest.mark.parametrize("num,den", [(196, 185), (185, 196), (3, 2), (2, 3)])
def test_tempo_then_resample_moves_the_pitch(num, den):
    x = tone()
    mid, n, _ = R.wsola_f32(x, None, den / num)
    y, _ = R64.resample64(mid, num, den)
    assert abs(len(y) - len(x)) <= 2
    f = peak_hz(y, 8192, 8192, lo=60.0, hi=260.0)
    print(f"{num} / {den}: peak {f:.3f} Hz, want {F_TONE * num / den:.3f}; {len(y)} samples of {len(x)}")
    assert abs(f - F_TONE * num / den) < 0.25


def test_tempo_sizes():
    assert audio.tempo_sizes(22050) == (1808, 265, 324)
    assert audio.tempo_sizes(16000) == (1312, 192, 235)
    assert audio.tempo_sizes(1000, 16.0, 8.0, 4.0) == (16, 4, 8)
    assert audio.tempo_sizes(48000, 170.0, 42.0, 42.0) == (8160, 2016, 2016)
    for bad in ((22050, 82.0, 14.68, 60.0), (22050, 400.0, 14.68, 12.0), (22050, 82.0, 100.0, 12.0), (22050, 82.0, 0.01, 12.0), (22050, 82.0, 14.68, 0.01),
                (0, 82.0, 14.68, 12.0), (22050, float("nan"), 14.68, 12.0), (22050, 82.0, -1.0, 12.0), (True, 82.0, 14.68, 12.0)):
        with pytest.raises(ValueError, match="tempo:"):
            audio.tempo_sizes(*bad)


def test_out_lengths_are_the_fp64_floor():
    assert ops.tempo_out_lengths([44100, 44100, 0, 1, 7], [0.85, 1.15, 1.0, 4.0, 0.25]).tolist() == [51882, 38347, 0, 0, 28]
    assert R.out_length(44100, 0.85) == 51882 and R.out_length(44100, 1.15) == 38347


def test_header_declares_and_lib_binds_the_entry_points():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    names = ("nsg_audio_tempo", "nsg_audio_tempo_workspace_bytes", "nsg_audio_mix_noise", "nsg_audio_mix_noise_workspace_bytes")
    for name in names:
        assert re.search(r"NSG_API\s+\w+\s+%s\s*\(" % name, text), name
        assert name in _lib.HEADER_SYMBOLS and hasattr(_lib.load(), name)
    sigs, consts, _ = _lib.parse_header(text)
    P, I32, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    assert sigs["nsg_audio_tempo"] == (I32, [P] * 6 + [I32] * 6 + [P, SZ, P])
    assert sigs["nsg_audio_tempo_workspace_bytes"] == (SZ, [I32] * 4)
    assert sigs["nsg_audio_mix_noise"] == (I32, [P] * 8 + [I32] * 3 + [P, SZ, P])
    assert sigs["nsg_audio_mix_noise_workspace_bytes"] == (SZ, [I32] * 2)
    assert consts["NSG_MIX_PARTIAL"] == R.MIX_PARTIAL == 4096


def test_size_queries():
    lib = _lib.load()
    assert lib.nsg_audio_tempo_workspace_bytes(3, 1000, 64, 8) >= 3 * 18 * 4
    assert lib.nsg_audio_tempo_workspace_bytes(0, 1000, 64, 8) == 0 and lib.nsg_audio_tempo_workspace_bytes(3, 1000, 8, 8) == 0
    assert lib.nsg_audio_mix_noise_workspace_bytes(3, 4097) >= 3 * 2 * 2 * 8 + 3 * 4
    assert lib.nsg_audio_mix_noise_workspace_bytes(3, 0) == 0


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)

    def tempo(wav=P, factor=P, out_lengths=P, out=P, positions=P, B=2, L=6000, L_out=7000, S=1808, O=265, W=324, ws=null, nb=0):
        return lib.nsg_audio_tempo(wav, null, factor, out_lengths, out, positions, B, L, L_out, S, O, W, ws, nb, None)

    for kw in (dict(wav=null), dict(factor=null), dict(out_lengths=null), dict(out=null), dict(B=0), dict(L=0), dict(L_out=0), dict(B=-1)):
        assert tempo(**kw) == -1 and b"nsg_audio_tempo" in lib.nsg_last_error_string(), kw
    unsupported = [dict(O=0), dict(O=2049, S=8192), dict(S=529), dict(S=8193), dict(W=0), dict(W=2049), dict(B=1 << 16, L_out=1 << 15),
                   dict(L=(1 << 31) - 1000)]
    for kw in unsupported:
        assert tempo(**kw) == -2 and b"outside" in lib.nsg_last_error_string(), kw
    need = lib.nsg_audio_tempo_workspace_bytes(2, 7000, 1808, 265)
    assert need >= 2 * 5 * 4
    for kw in (dict(positions=null), dict(positions=null, ws=P, nb=need - 1)):
        assert tempo(**kw) == -3 and b"workspace" in lib.nsg_last_error_string(), kw

    def mix(wav=P, noise=P, gain=P, level=P, offset=P, out=P, B=2, L=6000, Ln=100, ws=P, nb=1 << 20):
        return lib.nsg_audio_mix_noise(wav, null, noise, gain, level, offset, out, null, B, L, Ln, ws, nb, None)

    for kw in (dict(wav=null), dict(noise=null), dict(gain=null), dict(level=null), dict(offset=null), dict(out=null), dict(B=0), dict(L=0), dict(Ln=0)):
        assert mix(**kw) == -1 and b"nsg_audio_mix_noise" in lib.nsg_last_error_string(), kw
    assert mix(B=1 << 21, L=1 << 21, nb=1 << 62) == -2 and b"outside" in lib.nsg_last_error_string()
    need = lib.nsg_audio_mix_noise_workspace_bytes(2, 6000)
    for kw in (dict(ws=null), dict(nb=need - 1)):
        assert mix(**kw) == -3 and b"workspace" in lib.nsg_last_error_string(), kw


def test_wrappers_check_before_anything_is_launched():
    x = np.zeros(6000, dtype=np.float32)
    for kw in (dict(factor=0.2), dict(factor=4.5), dict(factor=float("nan")), dict(factor=[1.0, 1.0]), dict(factor="fast"), dict(factor=1.0, overlap_ms=60.0),
               dict(factor=1.0, sample_rate=0)):
        with pytest.raises(ValueError, match="tempo:"):
            audio.tempo(x, **kw)
    with pytest.raises(TypeError, match="tempo:"):
        audio.tempo(np.zeros((2, 6000), dtype=np.float32), 1.0)
    with pytest.raises(ValueError, match=r"every length must be in \[0, 6000\]"):
        audio.tempo(torch.zeros(2, 6000), 1.0, lengths=[6000, 6001])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        audio.tempo(torch.zeros(2, 6000), [0.9, 1.1])
    with pytest.raises(ValueError, match="resample:"):
        audio.pitch_shift(x, 0, 3)
    with pytest.raises(ValueError, match="needs a table"):
        audio.pitch_shift(x, 22051, 22050)
    with pytest.raises(ValueError, match="pitch_shift: den / num"):
        audio.pitch_shift(x, 5, 1)
    with pytest.raises(ValueError, match="pitch_shift: every clip"):
        audio.pitch_shift(torch.zeros(2, 6000), 2, 3, lengths=[6000, 1])
    noise = np.ones(100, dtype=np.float32)
    for kw in (dict(level=float("inf")), dict(offset=100), dict(offset=-1), dict(offset=1.5), dict(gain_db=float("nan")), dict(gain_db=4000.0),
               dict(level=[0.1, 0.2])):
        with pytest.raises(ValueError, match="mix_noise:"):
            audio.mix_noise(x, noise, **dict(dict(level=0.1, offset=0), **kw))
    for bad in (np.ones((2, 50), dtype=np.float32), np.ones(0, dtype=np.float32), np.ones(10, dtype=np.int16), [1.0, 2.0], torch.ones(10, dtype=torch.float64)):
        with pytest.raises(TypeError, match="mix_noise:"):
            audio.mix_noise(x, bad, 0.1, 0)
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        audio.mix_noise(torch.zeros(2, 6000), torch.ones(10), 0.1, 0)


def test_random_draws_reproduce_and_follow_the_documented_order():
    def gen(seed):
        return torch.Generator().manual_seed(seed)

    a = audio.augment_draws(5, gen(7), noise_len=1000)
    b = audio.augment_draws(5, gen(7), noise_len=1000)
    assert set(a) == {"tempo", "gain_db", "level", "offset"} and all(np.array_equal(a[k], b[k]) for k in a)
    u = torch.rand(20, dtype=torch.float64, generator=gen(7)).numpy().reshape(5, 4)             # tempo, gain, level, offset per clip
    assert np.array_equal(a["tempo"], 0.85 + (1.15 - 0.85) * u[:, 0]) and np.array_equal(a["gain_db"], -6.0 + 14.0 * u[:, 1])
    assert np.array_equal(a["level"], 0.5 * u[:, 2]) and np.array_equal(a["offset"], np.floor(u[:, 3] * 1000).astype(np.int64))
    assert a["offset"].dtype == np.int64 and (a["tempo"] >= 0.85).all() and (a["tempo"] < 1.15).all()
    c = audio.augment_draws(5, gen(7))                                                          # without noise: two draws a clip
    v = torch.rand(10, dtype=torch.float64, generator=gen(7)).numpy().reshape(5, 2)
    assert set(c) == {"tempo", "gain_db"} and np.array_equal(c["tempo"], 0.85 + (1.15 - 0.85) * v[:, 0])
    assert not np.array_equal(audio.augment_draws(5, gen(8))["tempo"], c["tempo"])
    g = gen(3)                                                                                   # the generator moves on: a second batch differs
    first, second = audio.augment_draws(2, g), audio.augment_draws(2, g)
    assert not np.array_equal(first["tempo"], second["tempo"])
    for kw in (dict(tempo_range=(0.1, 1.0)), dict(tempo_range=(1.2, 0.9)), dict(gain_range=(0.0,)), dict(noise_levels=(0.0, float("inf"))),
               dict(noise_len=0)):
        with pytest.raises(ValueError, match="augment:"):
            audio.augment_draws(2, gen(0), **kw)
    with pytest.raises(TypeError, match="generator"):
        audio.augment_draws(2, np.random.RandomState(0))


def test_random_augment_runs_tempo_then_mix_with_the_draws(monkeypatch):
    """With the two stages stubbed: the draws reach them in order, tempo first, its output lengths go on to the mix."""
    calls = []

    def fake_tempo(wav, factor, sample_rate=22050, lengths=None, **kw):
        calls.append(("tempo", np.array(factor), None if lengths is None else np.array(lengths)))
        return wav, np.array([10, 20], dtype=np.int32)

    def fake_mix(wav, noise, level, offset, gain_db=0.0, lengths=None, **kw):
        calls.append(("mix", np.array(level), np.array(offset), np.array(gain_db), np.array(lengths), len(noise)))
        return wav

    monkeypatch.setattr(audio, "tempo", fake_tempo)
    monkeypatch.setattr(audio, "mix_noise", fake_mix)
    wav = torch.zeros(2, 30)
    noise = np.ones(500, dtype=np.float32)
    out, out_lens, params = audio.random_augment(wav, [30, 25], torch.Generator().manual_seed(5), noise=noise)
    want = audio.augment_draws(2, torch.Generator().manual_seed(5), noise_len=500)
    assert [c[0] for c in calls] == ["tempo", "mix"] and out_lens.tolist() == [10, 20]
    assert np.array_equal(calls[0][1], want["tempo"]) and calls[0][2].tolist() == [30, 25]
    assert np.array_equal(calls[1][1], want["level"]) and np.array_equal(calls[1][2], want["offset"]) and np.array_equal(calls[1][3], want["gain_db"])
    assert calls[1][4].tolist() == [10, 20] and calls[1][5] == 500 and all(np.array_equal(params[k], want[k]) for k in want)
    del calls[:]
    audio.random_augment(wav, None, torch.Generator().manual_seed(5))                            # no noise: the gain alone, level 0
    assert calls[1][0] == "mix" and float(calls[1][1]) == 0.0 and calls[1][5] == 1


def test_mix_restatements_agree_and_the_order_is_the_named_one():
    rs = np.random.RandomState(2)
    x = rs.standard_normal(9000).astype(np.float32)
    noise = rs.standard_normal(700).astype(np.float32)
    o32, ex, en, s = R.mix_f32(x, 8500, noise, 0.7, 0.3, 699, L=9000)
    o64, ex64, en64, s64 = R.mix_f64(x, 8500, noise, 0.7, 0.3, 699, L=9000)
    assert o32.dtype == np.float32 and not o32[8500:].any()
    assert abs(ex - ex64) <= (8500 + 16) * 2.0 ** -52 * ex64 and abs(en - en64) <= (8500 + 16) * 2.0 ** -52 * en64
    assert abs(float(s) - s64) <= 2.0 ** -23 * s64
    # the gain's and s's rounding, the two products and the sum: five roundings of 2^-24 each, of which a term meets three
    assert np.abs(o32 - o64).max() <= 4 * 2.0 ** -24 * (np.abs(0.7 * x).max() + s64 * np.abs(noise).max())
    v = np.arange(1, 4098, dtype=np.float32)                       # 4097 samples: one partial and one sample; the integers' squares add exactly
    assert R.energy_in_order(v) == float(np.sum(v.astype(np.float64) ** 2))
    assert R.mix_f32(x, 0, noise, 0.7, 0.3, 0)[3] == 0.0 and R.mix_f32(x, 100, np.zeros(5, dtype=np.float32), 0.7, 0.3, 0)[3] == 0.0
