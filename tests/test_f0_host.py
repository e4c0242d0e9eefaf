"""CPU: the host side of the F0 feature -- the restatements the GPU tests hold the kernels to (tests/helpers/f0_ref.py), on signals
whose pitch is known; the header's declarations, their binding and their refusals; the argument checks that raise before any
kernel runs.

The bound on yin_f32 against yin_f64 (F0_BOUND below), with u = 2^-24.  A term fl(fl(x - y)^2) is off by at most 3 u relative and
a chain of W non-negative terms adds (W - 1) u: d(tau) within (W + 2) u.  c(tau) adds the group chain (7), the chain over at most
ng = ceil(tau_max / 8) group totals and one more add: within (W + ng + 10) u.  d' = fl(fl(d tau) / c) adds two roundings:
eps = (2 W + ng + 14) u relative, 1.3e-4 at the defaults.  With a, b, c = d' at tau* - 1, tau*, tau* + 1 off by eps each, the
numerator 0.5 (a - c) of delta moves by at most 0.5 eps (a + c) and the denominator a - 2b + c by eps (a + 2b + c); with
|delta| <= 0.5 that is |d delta| <= eps (a + b + c) / (a - 2b + c) to first order, plus 3 u for delta's own roundings.  F0 =
sr / (tau* + delta) turns it into d delta / (tau* + delta) relative, plus 2 u, and a relative change r is 1200 / ln 2 * r cents:
    bound = 1200 / ln 2 * (eps (a + b + c) / ((a - 2b + c) (tau* + delta)) + 5 u) * 1.01
the 1.01 for the second-order terms.  Measured (the four six-harmonic tones, 38 interior frames each, this summation order):
1.0e-4 .. 1.4e-4 cent against bounds of 1.2e-3 (70 Hz) .. 5.0e-3 (440 Hz) cent, 2 % .. 12 % of the bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, evaluate, models, ops
from tests.helpers import f0_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, W, HOP = 22050, 1024, 256
TAU_MIN, TAU_MAX = 45, 339
TONES = [70.0, 110.0, 220.0, 440.0]
U = 2.0 ** -24


def tone(freq, seconds=0.5, harmonics=6, sr=SR):
    n = np.arange(int(seconds * sr), dtype=np.float64)
    return sum(0.6 ** h * np.sin(2 * np.pi * freq * h * n / sr) for h in range(1, harmonics + 1)).astype(np.float32)


def interior(n, W=W, hop=HOP, tau_max=TAU_MAX):
    """Frames whose whole span [t hop - W/2, t hop + W/2 + tau_max) lies inside the clip."""
    t = np.arange(1 + n // hop)
    return t[(t * hop - W // 2 >= 0) & (t * hop + W // 2 + tau_max <= n)]


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, dtype=np.float64) / ref)


@pytest.fixture(scope="module")
def tracked():
    out = {}
    for f in TONES:
        x = tone(f)
        out[f] = (x, R.yin_f32(x), R.yin_f64(x, detail=True))
    return out


def test_lags_are_the_defaults():
    assert audio.f0_lags(SR, 65.0, 500.0) == (TAU_MIN, TAU_MAX)
    assert audio.f0_lags(16000, 80.0, 400.0) == (40, 200)
    for bad in ((SR, 0.0, 500.0), (SR, 500.0, 65.0), (SR, 20.0, 500.0), (0, 65.0, 500.0), (SR, float("nan"), 500.0)):
        with pytest.raises(ValueError, match="f0:"):
            audio.f0_lags(*bad)


@pytest.mark.parametrize("freq", TONES)
def test_pure_tones_fp32_against_fp64_and_the_truth(tracked, freq):
    x, (f32, ap32), (f64, ap64, lag, abc) = tracked[freq]
    assert f32.dtype == np.float32 and ap32.dtype == np.float32 and len(f32) == 1 + len(x) // HOP
    t = interior(len(x))
    assert len(t) >= 30
    assert np.array_equal(f32 > 0, f64 > 0), "the voiced decisions differ"          # every frame, the edges included
    assert (f32[t] > 0).all()
    print(f"{freq} Hz: d' <= {ap64[t].max():.4f} on interior frames (threshold 0.1)")
    assert ap64[t].max() < 0.01 and ap32[t].max() < 0.01                             # far from the decision
    off32, off64 = np.abs(cents(f32[t], freq)), np.abs(cents(f64[t], freq))
    print(f"{freq} Hz: |F0 - truth| <= {off32.max():.3f} cent (fp32), {off64.max():.3f} cent (fp64)")
    assert off32.max() < 1.0 and off64.max() < 1.0
    a, b, c = abc[t].T
    ng = -(-TAU_MAX // R.LAG_GROUP)
    eps = (2 * W + ng + 14) * U
    period = SR / f64[t]
    bound = 1200.0 / np.log(2.0) * (eps * (a + b + c) / ((a - 2 * b + c) * period) + 5 * U) * 1.01
    diff = np.abs(cents(f32[t], f64[t]))
    print(f"{freq} Hz: |F0_32 - F0_64| <= {diff.max():.3e} cent, bound {bound.min():.3e} .. {bound.max():.3e}, worst share {np.max(diff / bound):.3f}")
    assert np.isfinite(bound).all() and (diff <= bound).all()


def test_noise_and_silence_are_unvoiced():
    rs = np.random.RandomState(0)
    noise = (0.3 * rs.standard_normal(SR // 2)).astype(np.float32)
    for yin in (R.yin_f32, R.yin_f64):
        f, ap = yin(noise)
        t = interior(len(noise))
        assert not f.any() and ap[t].min() > 0.5, ap[t].min()
        f, ap = yin(np.zeros(6000, dtype=np.float32))
        assert not f.any() and (ap == 1.0).all()
    f, ap = R.yin_f32(np.zeros(6000, dtype=np.float32))
    assert (f.view(np.uint32) == 0).all()                                            # +0.0 by bit pattern


def test_tones_at_the_ends_of_the_lag_range():
    n = np.arange(SR // 2, dtype=np.float64)
    for period in (TAU_MIN, TAU_MAX):
        x = sum(0.6 ** h * np.sin(2 * np.pi * h * n / period) for h in range(1, 7)).astype(np.float32)
        t = interior(len(x))
        f32, _ = R.yin_f32(x)
        f64, _, lag, abc = R.yin_f64(x, detail=True)
        assert (lag[t] == period).all()
        if period == TAU_MAX:                                                        # no neighbour above: delta = 0, F0 = sr / tau exactly
            assert np.isnan(abc[t][:, 0]).all()
            assert (f32[t] == np.float32(SR) / np.float32(period)).all() and (f64[t] == SR / period).all()
        else:                                                                        # the neighbour below tau_min is defined and used
            assert np.isfinite(abc[t]).all()
            assert np.abs(cents(f32[t], SR / period)).max() < 1.0 and np.abs(cents(f64[t], SR / period)).max() < 1.0
    # a one-lag range: whatever is chosen is that lag, unrefined
    x = tone(220.5)                                                                  # period 100 samples
    f32, ap = R.yin_f32(x, tau_min=100, tau_max=100)
    t = interior(len(x))
    assert (f32[t] == np.float32(SR) / np.float32(100)).all()


def test_restatement_pads_rows_and_ignores_samples_past_the_length():
    x = tone(110.0, seconds=0.2)
    f_all, ap_all = R.yin_f32(x)
    poisoned = np.concatenate((x[:3000], np.full(1000, np.nan, dtype=np.float32)))
    f, ap = R.yin_f32(poisoned, n=3000, L=6000)
    want_f, want_ap = R.yin_f32(x[:3000])
    assert len(f) == 1 + 6000 // HOP and np.isfinite(f).all() and np.isfinite(ap).all()
    nb = 1 + 3000 // HOP
    assert np.array_equal(f[:nb], want_f) and np.array_equal(ap[:nb], want_ap) and not f[nb:].any() and (ap[nb:] == 1).all()
    assert np.array_equal(f_all[:4], want_f[:4])                                     # frames whose span ends before sample 3000


def test_path_stats_by_hand():
    fa = np.array([100.0, 0.0, 200.0, 400.0], dtype=np.float32)
    fb = np.array([200.0, 200.0, 0.0], dtype=np.float32)
    path = np.array([[0, 0], [1, 1], [2, 1], [3, 2], [3, 2]], dtype=np.int32)
    stats, mags = R.path_stats_f64(fa, fb, path, 3)                                  # cells (100, 200), (-, 200), (200, 200)
    x, y = np.log2([100.0, 200.0]), np.log2([200.0, 200.0])
    want = [3, 2, 0, 1, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(), 1.0]
    assert np.allclose(stats, want, rtol=1e-15, atol=0) and stats[9] == pytest.approx(1.0, abs=1e-14)
    assert mags[5] == pytest.approx(1.0, abs=1e-14)
    stats, _ = R.path_stats_f64(fa, fb, path, 5)                                     # + (400, -) twice
    assert stats[:4].tolist() == [5, 2, 2, 1]
    rmse, vuv, corr = (float(v) for v in audio.f0_figures(torch.from_numpy(stats)))
    assert rmse == pytest.approx(1200.0 * np.sqrt(0.5)) and vuv == pytest.approx(3 / 5) and np.isnan(corr)   # y is constant: 0 / 0
    one = audio.f0_figures(torch.tensor([[4.0, 1, 1, 2, 7, 7, 49, 49, 49, 0]], dtype=torch.float64))
    assert np.isnan(float(one[0])) and float(one[1]) == 0.75 and np.isnan(float(one[2]))                    # n_vv < 2


def test_header_declares_and_lib_binds_the_entry_points():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    for name in ("nsg_audio_f0", "nsg_f0_path_stats"):
        assert re.search(r"NSG_API\s+\w+\s+%s\s*\(" % name, text), name
        assert name in _lib.HEADER_SYMBOLS and hasattr(_lib.load(), name)
    sigs, consts, _ = _lib.parse_header(text)
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert sigs["nsg_audio_f0"] == (I32, [P] * 4 + [I32] * 6 + [F32] * 2 + [P])
    assert sigs["nsg_f0_path_stats"] == (I32, [P] * 5 + [I32] * 3 + [P])
    assert consts["NSG_F0_LAG_GROUP"] == R.LAG_GROUP == 8 and consts["NSG_VERSION"] == 104


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)

    def f0(wav=P, f=P, ap=P, B=2, L=6000, W=1024, hop=256, tmin=45, tmax=339, thr=0.1, sr=22050.0):
        return lib.nsg_audio_f0(wav, null, f, ap, B, L, W, hop, tmin, tmax, thr, sr, None)

    invalid = [dict(wav=null), dict(f=null), dict(ap=null), dict(B=0), dict(L=0), dict(W=0), dict(hop=0), dict(tmin=0), dict(tmax=0),
               dict(thr=0.0), dict(thr=1.5), dict(thr=float("nan")), dict(sr=0.0), dict(sr=-1.0)]
    for kw in invalid:
        assert f0(**kw) == -1 and b"nsg_audio_f0" in lib.nsg_last_error_string(), kw
    unsupported = [dict(W=1023), dict(W=62), dict(W=2050), dict(tmin=340), dict(tmax=1025), dict(B=1 << 20, L=1 << 20, hop=256)]
    for kw in unsupported:
        assert f0(**kw) == -2 and b"outside" in lib.nsg_last_error_string(), kw

    def stats(fa=P, fb=P, path=P, steps=P, out=P, B=2, Ta=10, Tb=12):
        return lib.nsg_f0_path_stats(fa, fb, path, steps, out, B, Ta, Tb, None)

    for kw in (dict(fa=null), dict(fb=null), dict(path=null), dict(steps=null), dict(out=null), dict(B=0), dict(Ta=0), dict(Tb=0)):
        assert stats(**kw) == -1 and b"nsg_f0_path_stats" in lib.nsg_last_error_string(), kw
    assert stats(Ta=1 << 30, Tb=5) == -2 and b"outside" in lib.nsg_last_error_string()


def test_wrappers_check_before_anything_is_launched():
    x = np.zeros(6000, dtype=np.float32)
    for kw in (dict(frame_length=1023), dict(frame_length=32), dict(frame_length=4096), dict(frame_length=1024.0), dict(hop_size=0),
               dict(threshold=0.0), dict(threshold=1.01), dict(fmin=10.0), dict(fmin=600.0), dict(fmax=0.0)):
        with pytest.raises(ValueError, match="f0:"):
            audio.f0(x, **kw)
    with pytest.raises(TypeError, match="f0:"):
        audio.f0(np.zeros((2, 6000), dtype=np.float32))
    with pytest.raises(ValueError, match="lengths"):
        audio.f0(x, lengths=[6000])
    with pytest.raises(ValueError, match=r"every length must be in \[0, 6000\]"):
        audio.f0(torch.zeros(2, 6000), lengths=[6000, 6001])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        audio.f0(torch.zeros(2, 6000))
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.f0_path_stats(torch.zeros(2, 10), torch.zeros(2, 12), torch.zeros(2, 21, 2, dtype=torch.int32), torch.ones(2, dtype=torch.int32))
    plain = models.VQVAE(1, 16, 32)
    with pytest.raises(ValueError, match="no speaker embedding"):
        evaluate.test_conversion_f0(None, plain, [], torch.device("cpu"), 0)
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.test_conversion_f0(None, models.VQVAE(1, 16, 32, n_speakers=2), [], torch.device("cpu"), 0)
