"""CPU: the host side of the PSOLA pitch shifter -- the restatement the GPU tests hold the kernels to (tests/helpers/
psola_ref.py) on signals whose answer is known: the identity, one mark per pulse, the pitch that must move while the strongest
harmonic stays near the resonance; the envelope arithmetic; the header's declarations, their binding and their refusals; the
argument checks that raise before any kernel runs; the random draws."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, ops
from tests.helpers import psola_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, HOP = 22050, 256
P_U, P_MIN, P_MAX = 110, 45, 339


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def acf_f0(y, sr=SR, lo=60.0, hi=400.0):
    """The F0 of a steady signal from the peak of its autocorrelation, refined by a parabola."""
    y = np.asarray(y, dtype=np.float64)
    n = 1 << int(np.ceil(np.log2(2 * len(y))))
    r = np.fft.irfft(np.abs(np.fft.rfft(y, n)) ** 2)[:len(y)]
    a, b = int(sr / hi), int(sr / lo)
    k = a + int(np.argmax(r[a:b]))
    d = 0.5 * (r[k - 1] - r[k + 1]) / (r[k - 1] - 2 * r[k] + r[k + 1])
    return sr / (k + d)


def strongest_harmonic(y, sr=SR, lo=500.0, hi=1600.0):
    nfft = 1 << 17
    sp = np.abs(np.fft.rfft(np.asarray(y, dtype=np.float64) * np.hanning(len(y)), nfft))
    a, b = int(lo * nfft / sr), int(hi * nfft / sr)
    return (a + int(np.argmax(sp[a:b]))) * sr / nfft


@pytest.fixture(scope="module")
def vowel110():
    x, voiced = R.vowel(110.0, 0.6)
    return x, R.track(voiced, 110.0, HOP)


def run(x, f, f_out, dtype=np.float32, n=None):
    return R.psola_ref(x, len(x) if n is None else n, f, f_out, HOP, SR, P_U, P_MIN, P_MAX, dtype=dtype)


def test_constants_agree_with_the_package_and_the_header():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    _, consts, _ = _lib.parse_header(text)
    assert consts["NSG_PSOLA_MIN_WEIGHT_LOG2"] == 10 and R.MIN_WEIGHT == ops.PSOLA_MIN_WEIGHT == 2.0 ** -10
    assert audio.psola_periods(SR) == (P_U, P_MIN, P_MAX) and audio.PSOLA_ALPHA == R.ALPHA
    assert ops.PSOLA_MAX_PERIOD == audio.F0_MAX_LAG


def test_one_mark_per_pulse_on_the_pulses(vowel110):
    x, f = vowel110
    marks = R.marks_ref(x, len(x), f, HOP, SR, P_U, P_MIN, P_MAX)
    gaps = np.diff(marks)[1:-1]                                                 # (the first pulse comes after a period of zeros; the end cuts the last range)
    assert abs(len(marks) - 0.6 * 110) <= 1 and gaps.min() >= 199 and gaps.max() <= 202          # 22050 / 110 = 200.45
    assert all(x[m] == x[m - 50:m + 51].max() for m in marks[1:-1])


def test_identity_is_exact_outside_the_marks_and_within_the_bound_between(vowel110):
    x, f = vowel110
    for track in (f, np.zeros_like(f)):                                         # voiced, and the all-unvoiced pass-through
        r = run(x, track, track)
        assert r["syn"] == r["marks"] and r["map"] == list(range(len(r["marks"])))
        m0, m1 = r["marks"][0], r["marks"][-1]
        assert np.array_equal(bits(r["out"][:m0 + 1]), bits(x[:m0 + 1])) and np.array_equal(bits(r["out"][m1:]), bits(x[m1:]))
        assert np.array_equal(bits(r["out"][r["marks"]]), bits(x[r["marks"]]))
        r64 = run(x, track, track, np.float64)
        bound = R.fp32_bound(r64["den"], r64["grains"], float(np.abs(x).max()))
        assert (np.abs(r["out"].astype(np.float64) - x) <= bound).all() and np.abs(r64["out"] - x).max() < 1e-15
        assert abs(r64["den"][m0:m1 + 1] - 1.0).max() < 1e-12                                     # w(u) + w(1 - u) = 1
    unvoiced = R.marks_ref(x, len(x), np.zeros_like(f), HOP, SR, P_U, P_MIN, P_MAX)
    assert (np.diff(unvoiced) == P_U).all() and unvoiced[0] == R.argmax_key(x, 0, P_U - 1)


@pytest.mark.parametrize("ratio", [0.8, 1.25])
def test_the_pitch_moves_and_the_resonance_stays(vowel110, ratio):
    x, f = vowel110
    r = run(x, f, (f * np.float32(ratio)).astype(np.float32))
    y = r["out"][2000:-2000]
    assert abs(acf_f0(y) - 110.0 * ratio) < 1.5
    assert abs(strongest_harmonic(y) - 1000.0) < 110.0 * ratio                  # within a harmonic spacing of the resonance
    t = np.arange(len(y)) * ratio                                               # plain resampling moves it with the pitch
    z = np.interp(t[t < len(x) - 1], np.arange(len(x)), x)
    assert abs(strongest_harmonic(z) - 1000.0 * ratio) < 110.0 * ratio and abs(strongest_harmonic(z) - 1000.0) > 150.0
    assert len(r["out"]) == len(x)


def test_fp32_and_fp64_restatements_agree_within_the_derived_bound(vowel110):
    x, f = vowel110
    f_out = (f * np.float32(1.25)).astype(np.float32)
    a, b = run(x, f, f_out), run(x, f, f_out, np.float64)
    assert a["marks"] == b["marks"] and a["syn"] == b["syn"]
    safe = np.abs(b["den"] - R.MIN_WEIGHT) > 1e-5
    bound = R.fp32_bound(b["den"], b["grains"], float(np.abs(x).max()))
    assert (np.abs(a["out"] - b["out"])[safe] <= bound[safe]).all() and np.median(bound[bound > 0]) < 1e-5


def test_ties_short_clips_and_hostile_tracks():
    x = np.zeros(3000, dtype=np.float32)
    x[100:104] = 1.0                                                            # a flat-topped pulse: the smallest index
    x[300:303] = 1.0
    f = np.full(1 + 3000 // HOP, 110.0, dtype=np.float32)
    marks = R.marks_ref(x, 3000, f, HOP, SR, P_U, P_MIN, P_MAX)
    assert marks[0] == 100 and marks[1] == 300
    assert R.marks_ref(x, 0, f, HOP, SR, P_U, P_MIN, P_MAX) == [] and R.marks_ref(x, 1, f, HOP, SR, P_U, P_MIN, P_MAX) == [0]
    assert R.marks_ref(x, 150, f, HOP, SR, P_U, P_MIN, P_MAX) == [100]          # shorter than one period
    for v, want in ((np.nan, -P_U), (-5.0, -P_U), (0.0, -P_U), (np.inf, P_MIN), (1e30, P_MIN), (1e-30, P_MAX), (110.0, 200)):
        assert R.period(v, SR, P_U, P_MIN, P_MAX) == want, v
    for v in (np.nan, np.inf, -np.inf, -1.0, 1e-30, 1e30):
        r = run(x, np.full_like(f, v), np.full_like(f, 100.0))
        assert all(0 <= m < 3000 for m in r["marks"]) and np.isfinite(r["out"]).all()
        r = run(x, f, np.full_like(f, v))
        assert np.isfinite(r["out"]).all() and len(r["syn"]) <= R.sizes(3000, P_MIN, P_MAX)[4]


def test_envelope_arithmetic():
    assert R.sizes(13230, P_MIN, P_MAX) == ops.psola_sizes(13230, P_MIN, P_MAX, (1, 4)) == (34, 390, 423, 9, 1470)
    assert ops.psola_sizes(1, 2, 2, (1, 2)) == (1, 1, 3, 1, 1)
    rng = np.random.default_rng(0)
    for _ in range(20):                                                         # marks are at least G apart, at most H_max
        x = rng.standard_normal(4000).astype(np.float32)
        f = rng.choice([0.0, 70.0, 200.0, 480.0, 1e9], size=1 + 4000 // HOP).astype(np.float32)
        marks = R.marks_ref(x, 4000, f, HOP, SR, P_U, P_MIN, P_MAX)
        G, K_max, H_max, Gs, J_max = R.sizes(4000, P_MIN, P_MAX)
        assert np.diff(marks).min() >= G and np.diff(marks).max() <= H_max and len(marks) <= K_max
        syn, _ = R.syn_ref(marks, f, (f * rng.choice([0.1, 0.5, 2.0, 10.0])).astype(np.float32), HOP, P_U, P_MIN, P_MAX)
        assert np.diff(syn).min() >= Gs and len(syn) <= J_max


def test_header_declares_and_lib_binds_the_entry_points():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    for name in ("nsg_audio_pitch_marks", "nsg_audio_psola"):
        assert re.search(r"NSG_API\s+\w+\s+%s\s*\(" % name, text), name
        assert name in _lib.HEADER_SYMBOLS and hasattr(_lib.load(), name)
    sigs, _, _ = _lib.parse_header(text)
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert sigs["nsg_audio_pitch_marks"] == (I32, [P] * 5 + [I32] * 4 + [F32] + [I32] * 6 + [P])
    assert sigs["nsg_audio_psola"] == (I32, [P] * 10 + [I32] * 4 + [F32] + [I32] * 7 + [P])
    assert not [n for n in sigs if "psola" in n and n.endswith("workspace_bytes")]


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)

    def marks(wav=P, f0=P, out=P, cnt=P, B=2, L=13230, T=52, hop=256, sr=22050.0, Pu=110, Pmin=45, Pmax=339, an=1, ad=4, K=390, J=None):
        return lib.nsg_audio_pitch_marks(wav, null, f0, out, cnt, B, L, T, hop, sr, Pu, Pmin, Pmax, an, ad, K, None)

    def psola(wav=P, f0=P, fo=P, mk=P, nm=P, syn=P, mp=P, ns=P, out=P, B=2, L=13230, T=52, hop=256, sr=22050.0, Pu=110, Pmin=45, Pmax=339, an=1, ad=4,
              K=390, J=1470):
        return lib.nsg_audio_psola(wav, null, f0, fo, mk, nm, syn, mp, ns, out, B, L, T, hop, sr, Pu, Pmin, Pmax, an, ad, K, J, None)

    shared_invalid = [dict(wav=null), dict(f0=null), dict(B=0), dict(L=0), dict(T=0), dict(hop=0), dict(sr=0.0), dict(sr=float("inf")),
                      dict(sr=float("nan")), dict(Pu=0), dict(an=-1), dict(ad=0), dict(K=389)]
    shared_unsupported = [dict(hop=15), dict(hop=(1 << 20) + 1), dict(Pmin=1), dict(Pmin=340), dict(Pmax=1025), dict(an=3), dict(ad=(1 << 20) + 1),
                          dict(B=1 << 16, L=1 << 15, K=1 << 15, J=1 << 15), dict(B=1, L=(1 << 31) - 1000, K=1 << 30, J=1 << 30)]
    for fn, name, more in ((marks, b"nsg_audio_pitch_marks", [dict(out=null), dict(cnt=null)]),
                           (psola, b"nsg_audio_psola", [dict(fo=null), dict(mk=null), dict(nm=null), dict(syn=null), dict(mp=null), dict(ns=null),
                                                        dict(out=null), dict(J=1469)])):
        for kw in shared_invalid + more:
            assert fn(**kw) == -1 and lib.nsg_last_error_string().startswith(name), kw
        for kw in shared_unsupported:
            assert fn(**kw) == -2 and lib.nsg_last_error_string().startswith(name), kw


def test_wrappers_check_before_anything_is_launched():
    x, f = np.zeros(6000, dtype=np.float32), np.zeros(24, dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one of ratio and target_f0"):
        audio.pitch_shift_psola(x, f)
    with pytest.raises(ValueError, match="exactly one of ratio and target_f0"):
        audio.pitch_shift_psola(x, f, ratio=1.0, target_f0=f)
    for kw in (dict(ratio=0.4), dict(ratio=2.5), dict(ratio=float("nan")), dict(ratio=[1.0, 1.0]), dict(ratio="up"), dict(ratio=1.0, hop_size=8),
               dict(ratio=1.0, hop_size=256.0), dict(ratio=1.0, sample_rate=0), dict(ratio=1.0, fmin=10.0), dict(ratio=1.0, fmax=30000.0),
               dict(target_f0=np.zeros(23, dtype=np.float32))):
        with pytest.raises(ValueError, match="pitch_shift_psola:|psola:|f0:"):
            audio.pitch_shift_psola(x, f, **kw)
    for bad in (np.zeros((2, 24), dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(24, dtype=np.int32), [0.0] * 24, torch.zeros(1, 24)):
        with pytest.raises(TypeError, match="pitch_shift_psola:"):
            audio.pitch_shift_psola(x, bad, ratio=1.0)
        with pytest.raises(TypeError, match="pitch_marks:"):
            audio.pitch_marks(x, bad)
    with pytest.raises(TypeError, match="pitch_shift_psola:"):
        audio.pitch_shift_psola(torch.zeros(2, 6000), torch.zeros(3, 24), ratio=1.0)
    with pytest.raises(ValueError, match=r"every length must be in \[0, 6000\]"):
        audio.pitch_shift_psola(torch.zeros(2, 6000), torch.zeros(2, 24), ratio=1.0, lengths=[6000, 6001])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        audio.pitch_shift_psola(torch.zeros(2, 6000), torch.zeros(2, 24), ratio=[0.9, 1.1])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        audio.pitch_marks(torch.zeros(2, 6000), torch.zeros(2, 24))
    g = torch.Generator().manual_seed(0)
    for kw in (dict(semitones=(-13.0, 0.0)), dict(semitones=(2.0, 1.0)), dict(tracker="crepe"), dict(tracker_options=dict(hop=256)),
               dict(tracker_options=dict(hop_size=4)), dict(sample_rate=-1)):
        with pytest.raises(ValueError, match="perturb_pitch:|psola:|f0:"):
            audio.perturb_pitch(torch.zeros(2, 6000), None, g, **kw)
    with pytest.raises(TypeError, match="perturb_pitch:"):
        audio.perturb_pitch(x, None, g)
    with pytest.raises(TypeError, match="perturb_pitch:"):
        audio.perturb_pitch(torch.zeros(2, 6000), None, torch.manual_seed)
    assert torch.equal(g.get_state(), torch.Generator().manual_seed(0).get_state())               # a refused call draws nothing


def test_pitch_draws_reproduce_and_follow_the_documented_order():
    def gen(seed):
        return torch.Generator().manual_seed(seed)

    a, b = audio.pitch_draws(6, gen(5)), audio.pitch_draws(6, gen(5))
    assert set(a) == {"semitones", "ratio"} and all(np.array_equal(a[k], b[k]) for k in a)
    u = torch.rand(6, dtype=torch.float64, generator=gen(5)).numpy()
    assert np.array_equal(a["semitones"], -4.0 + 8.0 * u) and np.array_equal(a["ratio"], 2.0 ** (a["semitones"] / 12.0))
    assert not np.array_equal(audio.pitch_draws(6, gen(6))["ratio"], a["ratio"])
    g = gen(1)
    assert not np.array_equal(audio.pitch_draws(2, g)["ratio"], audio.pitch_draws(2, g)["ratio"])
    assert np.array_equal(audio.pitch_draws(3, gen(2), (12.0, 12.0))["ratio"], np.full(3, 2.0))
