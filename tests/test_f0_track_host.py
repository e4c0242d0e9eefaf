"""CPU: the path finder over YIN candidates (include/nsg.h: nsg_audio_f0_candidates, nsg_f0_viterbi) as its host restatements
state it (tests/helpers/f0_track_ref.py), and the refusals of the new entry points and wrappers before anything is launched.

  * the prototype signal: raw YIN makes octave errors and dropouts on it, the tracker makes neither and voices nothing of the
    noise tail, at the default unvoiced_cost and at both ends of its window; the fp32 and fp64 recurrences choose the same path;
  * hand-built candidate tensors with exactly representable costs: the tie rules, one frame, a frame without candidates, no
    frames, all unvoiced, a free voicing switch;
  * the candidate rule: silence, a pure tone, more than 8 minima, a plateau, a minimum at tau_max, tau_min = 1."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, evaluate, models, ops
from tests.helpers import f0_ref as R
from tests.helpers import f0_track_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_COSTS = dict(octave_cost=0.01, jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3)


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, dtype=np.float64) / ref)


@pytest.fixture(scope="module")
def prototype():
    x, f, sr, W, hop, tau_min, tau_max = K.prototype_signal()
    voiced, tail = K.prototype_frames(len(x), sr, W, hop)
    truth = f[np.minimum(np.arange(len(voiced)) * hop, len(x) - 1)]
    raw, _ = R.yin_f32(x, None, W, hop, tau_min, tau_max, 0.1, float(sr))
    cand32 = K.candidates_f32(x, None, W, hop, tau_min, tau_max, float(sr))
    cand64 = K.candidates_f64(x, None, W, hop, tau_min, tau_max, float(sr))
    return dict(x=x, sr=sr, tau_min=tau_min, voiced=voiced, tail=tail, truth=truth, raw=raw, cand32=cand32, cand64=cand64)


def errors(f0, p):
    """(gross errors, dropouts) among the voiced frames, frames voiced in the tail."""
    v = p["voiced"]
    on = f0 > 0
    off = np.abs(cents(np.where(on, f0, p["truth"]), p["truth"]))
    return int((v & on & (off > 50.0)).sum()), int((v & ~on).sum()), int((p["tail"] & on).sum())


def test_the_prototype_signal_is_the_issues(prototype):
    assert int(prototype["voiced"].sum()) == 106 and len(prototype["voiced"]) == 138
    assert int(prototype["tail"].sum()) > 10


def test_raw_yin_makes_octave_errors_and_dropouts(prototype):
    gross, drop, _ = errors(prototype["raw"], prototype)
    print("raw YIN at 0.1: gross errors", gross, "dropouts", drop)
    assert gross >= 1 and drop >= 1


@pytest.mark.parametrize("unvoiced_cost", [0.3, 0.2, 0.45])
def test_the_tracker_makes_neither_and_leaves_the_tail_unvoiced(prototype, unvoiced_cost):
    costs = dict(DEFAULT_COSTS, unvoiced_cost=unvoiced_cost)
    top = np.log2(prototype["sr"] / prototype["tau_min"])
    cf, ca, cl, cnt = prototype["cand32"]
    s32, c32, f32, a32 = K.viterbi_f32(cl, ca, cf, cnt, None, top, **costs)
    assert errors(f32, prototype) == (0, 0, 0)
    cf, ca, cl, cnt = prototype["cand64"]
    s64, c64, f64, a64 = K.viterbi_f64(cl, ca, cf, cnt, None, top, **costs)
    assert errors(f64, prototype) == (0, 0, 0)
    assert np.array_equal(s32, s64)                     # the same candidates (checked below) and the same path
    assert abs(float(c32) - float(c64)) < 1e-3 * float(c64)


def test_fp32_and_fp64_candidates_agree_on_the_prototype(prototype):
    (f32, a32, l32, n32), (f64, a64, l64, n64) = prototype["cand32"], prototype["cand64"]
    assert np.array_equal(n32, n64)
    assert np.allclose(f32, f64, rtol=1e-4) and np.allclose(a32, a64, atol=1e-4) and np.allclose(l32, l64, atol=1e-4)


@pytest.mark.parametrize("name", sorted(K.hand_cases()))
def test_hand_built_paths(name):
    logf, ap, f0, count, frames, costs, states, cost = K.hand_cases()[name]
    for fn, ft in ((K.viterbi_f32, np.float32), (K.viterbi_f64, np.float64)):
        s, c, f, a = fn(logf, ap, f0, count, frames, **costs)
        assert s.tolist() == states and float(c) == cost and type(c) is ft, (fn.__name__, s.tolist(), float(c))
        for t, st in enumerate(states):
            want_f = f0[t, st - 1] if st > 0 else 0.0
            want_a = ap[t, st - 1] if st > 0 else (1.0 if st < 0 or count[t] == 0 else ap[t, :count[t]].min())
            assert f[t] == want_f and a[t] == want_a, (t, st, f[t], a[t])


def test_slots_past_count_and_counts_outside_the_range_do_not_matter():
    rs = np.random.RandomState(3)
    T = 12
    logf, ap = rs.uniform(6, 9, (T, 8)).astype(np.float32), rs.uniform(0, 1, (T, 8)).astype(np.float32)
    f0, count = np.exp2(logf), rs.randint(0, 9, T).astype(np.int32)
    want = K.viterbi_f32(logf, ap, f0, count, None, 9.0)
    junk = [a.copy() for a in (logf, ap, f0)]
    for t in range(T):
        for a in junk:
            a[t, count[t]:] = np.nan
    wide = count.copy()
    wide[count == 8] = 11
    wide[count == 0] = -3
    got = K.viterbi_f32(*junk, wide, None, 9.0)
    for w, g in zip(want, got):
        assert np.array_equal(np.asarray(w).view(np.uint32), np.asarray(g).view(np.uint32))


# ---- the candidate rule --------------------------------------------------------------------------------------------------------
SMALL = dict(W=64, hop=16, tau_min=2, tau_max=40, sample_rate=8000.0)


def test_a_frame_of_zeros_has_no_candidate():
    cf, ca, cl, cnt = K.candidates_f32(np.zeros(200, dtype=np.float32), **SMALL)
    assert not cnt.any() and not cf.any() and not cl.any() and (ca == 1).all()
    assert all((dp[1:] == 1).all() for dp in K.dprime_f32(np.zeros(200, dtype=np.float32), **SMALL))


def test_dprime_is_yin_f32s():
    """The recorded d' is what yin_f32 searched: searching it again gives yin_f32's result, bit for bit."""
    x, _, sr, W, hop, tau_min, tau_max = K.prototype_signal()
    x = x[:6000]
    f0, ap = R.yin_f32(x, None, W, hop, tau_min, tau_max, 0.1, float(sr))
    rows = K.dprime_f32(x, None, W, hop, tau_min, tau_max, float(sr))
    again = [R._pick(dp, tau_min, tau_max, np.float32(0.1), np.float32(sr), np.float32)[:2] for dp in rows]
    assert np.array_equal(np.array([a[0] for a in again]).view(np.uint32), f0.view(np.uint32))
    assert np.array_equal(np.array([a[1] for a in again]).view(np.uint32), ap.view(np.uint32))


def test_a_pure_tones_candidates_are_its_period_and_multiples():
    sr, period = 22050.0, 63.0
    x = np.sin(2 * np.pi * np.arange(8000) / period).astype(np.float32)
    cf, ca, cl, cnt, lags = K.candidates_f32(x, sample_rate=sr, lags=True)
    f0, ap = R.yin_f32(x, sample_rate=sr)
    for t in range(4, len(cnt) - 4):                   # frames wholly inside the tone
        assert lags[t, :cnt[t]].tolist() == [63, 126, 189, 252, 315], (t, lags[t])
        assert cf[t, 0].view(np.uint32) == f0[t].view(np.uint32) and ca[t, 0].view(np.uint32) == ap[t].view(np.uint32)
        assert cl[t, 0] == np.float32(np.log2(np.float64(cf[t, 0])))
        assert abs(cents(cf[t, 0], sr / period)) < 1.0


def test_more_than_8_minima_keeps_the_8_smallest_in_lag_order():
    x = np.random.RandomState(5).standard_normal(4000).astype(np.float32)
    cf, ca, cl, cnt, lags = K.candidates_f32(x, lags=True)
    rows = K.dprime_f32(x)
    seen = 0
    for t, dp in enumerate(rows):
        minima = [tau for tau in range(45, 340) if dp[tau] < dp[tau - 1] and (tau == 339 or dp[tau] <= dp[tau + 1]) and dp[tau] < 1]
        if len(minima) > 8:
            seen += 1
            keep = sorted(sorted(minima, key=lambda tau: (dp[tau], tau))[:8])
            assert cnt[t] == 8 and lags[t].tolist() == keep and (np.diff(lags[t]) > 0).all()
            assert max(dp[tau] for tau in keep) <= min(dp[tau] for tau in minima if tau not in keep)
    assert seen >= 3


def test_plateau_end_of_range_and_tau_min_1():
    f32 = np.float32
    dp = np.array([0, 1.0, 0.9, 0.5, 0.5, 0.5, 0.7, 0.6, 0.6, 0.4], dtype=f32)          # d'(0 .. 9), tau_max = 9
    rows, lags = K.frame_candidates(dp, 1, 9, 100.0, f32)
    assert lags == [3, 7, 9]                           # each plateau's first lag (not 4, 5 or 8: 0.5 is not < 0.5); the minimum at tau_max
    assert rows[2][0] == f32(100.0) / f32(9.0) and rows[2][1] == f32(0.4)               # no parabola at tau_max
    assert rows[0][1] == f32(0.5)
    # tau_min = 1: lag 1 has no left neighbour and is never a candidate; lag 2 is one where d'(2) < d'(1)
    rows, lags = K.frame_candidates(np.array([0, 1.0, 0.25, 0.5, 0.75], dtype=f32), 1, 4, 100.0, f32)
    assert lags == [2] and rows[0][0] == f32(100.0) / (f32(2.0) + (f32(0.5) * f32(0.5)) / f32(1.0))
    # the left neighbour below tau_min is used: d'(3) < d'(2) although tau_min = 3; and a minimum that is not < 1 is none
    assert K.frame_candidates(np.array([0, 1.0, 0.75, 0.5, 0.75], dtype=f32), 3, 4, 100.0, f32)[1] == [3]
    assert K.frame_candidates(np.array([0, 1.0, 1.5, 1.0, 1.25], dtype=f32), 2, 4, 100.0, f32)[1] == []


# ---- the ABI and the wrappers --------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    for name in ("nsg_audio_f0_candidates", "nsg_f0_viterbi", "nsg_f0_viterbi_workspace_bytes"):
        assert re.search(r"NSG_API\s+\w+\s+%s\s*\(" % name, text), name
        assert name in _lib.HEADER_SYMBOLS and hasattr(_lib.load(), name)
    sigs, consts, _ = _lib.parse_header(text)
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert sigs["nsg_audio_f0_candidates"] == (I32, [P] * 6 + [I32] * 6 + [F32] + [P])
    assert sigs["nsg_f0_viterbi"] == (I32, [P] * 9 + [I32] * 2 + [F32] * 5 + [P, ctypes.c_size_t, P])
    assert sigs["nsg_f0_viterbi_workspace_bytes"] == (ctypes.c_size_t, [I32, I32])
    assert consts["NSG_F0_MAX_CANDIDATES"] == K.MAX_CANDIDATES == ops.F0_MAX_CANDIDATES == 8
    assert consts["NSG_F0_VITERBI_LDS_FRAMES"] == ops.F0_VITERBI_LDS_FRAMES


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)

    def cand(wav=P, cf=P, ca=P, cl=P, cnt=P, B=2, L=6000, W=1024, hop=256, tmin=45, tmax=339, sr=22050.0):
        return lib.nsg_audio_f0_candidates(wav, null, cf, ca, cl, cnt, B, L, W, hop, tmin, tmax, sr, None)

    invalid = [dict(wav=null), dict(cf=null), dict(ca=null), dict(cl=null), dict(cnt=null), dict(B=0), dict(L=0), dict(W=0), dict(hop=0),
               dict(tmin=0), dict(tmax=0), dict(sr=0.0), dict(sr=-1.0), dict(sr=float("nan")), dict(sr=float("inf"))]
    for kw in invalid:
        assert cand(**kw) == -1 and b"nsg_audio_f0_candidates" in lib.nsg_last_error_string(), kw
    for kw in (dict(W=1023), dict(W=62), dict(W=2050), dict(tmin=340), dict(tmax=1025), dict(B=1 << 20, L=1 << 20, hop=256)):
        assert cand(**kw) == -2 and b"outside" in lib.nsg_last_error_string(), kw

    big = ops.F0_VITERBI_LDS_FRAMES + 1

    def vit(lf=P, ca=P, cf=P, cnt=P, st=P, cost=P, f=P, ap=P, B=2, T=100, top=9.0, oc=0.01, jc=0.35, vc=0.14, uc=0.3, ws=null, nb=0):
        return lib.nsg_f0_viterbi(lf, ca, cf, cnt, null, st, cost, f, ap, B, T, top, oc, jc, vc, uc, ws, nb, None)

    nan, inf = float("nan"), float("inf")
    invalid = [dict(lf=null), dict(ca=null), dict(cf=null), dict(cnt=null), dict(st=null), dict(cost=null), dict(f=null), dict(ap=null),
               dict(B=0), dict(T=0), dict(top=nan), dict(top=inf), dict(top=-inf)]
    invalid += [{k: v} for k in ("oc", "jc", "vc", "uc") for v in (-0.25, nan, inf)]
    for kw in invalid:
        assert vit(**kw) == -1 and b"nsg_f0_viterbi" in lib.nsg_last_error_string(), kw
    assert vit(B=1 << 20, T=1 << 11) == -2 and b"outside" in lib.nsg_last_error_string()
    # the workspace: none up to NSG_F0_VITERBI_LDS_FRAMES frames, the back-pointers' beyond; one byte less is refused
    assert lib.nsg_f0_viterbi_workspace_bytes(3, ops.F0_VITERBI_LDS_FRAMES) == 0
    need = lib.nsg_f0_viterbi_workspace_bytes(3, big)
    assert need >= 3 * ((big + 7) // 8) * 9 * 4 and need % 256 == 0
    for kw in (dict(ws=P, nb=need - 1), dict(ws=P, nb=0), dict(ws=null, nb=need)):
        assert vit(B=3, T=big, **kw) == -3 and b"nsg_f0_viterbi: workspace too small" in lib.nsg_last_error_string(), kw


def test_wrappers_check_before_anything_is_launched():
    x = np.zeros(6000, dtype=np.float32)
    for fn, tag in ((audio.f0_candidates, "f0_candidates:"), (audio.f0_track, "f0_track:")):
        for kw in (dict(frame_length=1023), dict(frame_length=32), dict(frame_length=4096), dict(frame_length=1024.0), dict(hop_size=0)):
            with pytest.raises(ValueError, match=tag):
                fn(x, **kw)
        for kw in (dict(fmin=10.0), dict(fmin=600.0), dict(fmax=0.0)):
            with pytest.raises(ValueError, match="f0:"):
                fn(x, **kw)
        with pytest.raises(TypeError, match=tag):
            fn(np.zeros((2, 6000), dtype=np.float32))
        with pytest.raises(ValueError, match="lengths"):
            fn(x, lengths=[6000])
        with pytest.raises(ValueError, match=r"every length must be in \[0, 6000\]"):
            fn(torch.zeros(2, 6000), lengths=[6000, 6001])
        with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
            fn(torch.zeros(2, 6000))
    for kw in (dict(octave_cost=-0.1), dict(jump_cost=float("nan")), dict(vuv_cost=float("inf")), dict(unvoiced_cost="0.3")):
        with pytest.raises(ValueError, match="f0_track: .*finite number >= 0"):
            audio.f0_track(x, **kw)
    z = torch.zeros(2, 10, 8)
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.f0_viterbi(z, z, z, torch.zeros(2, 10, dtype=torch.int32), 9.0, 0.01, 0.35, 0.14, 0.3)
    model = models.VQVAE(1, 16, 32, n_speakers=2)
    with pytest.raises(ValueError, match="tracker must be 'yin' or 'viterbi'"):
        evaluate.test_conversion_f0(None, model, [], torch.device("cpu"), 0, tracker="pyin")
    with pytest.raises(ValueError, match="tracker_options"):
        evaluate.test_conversion_f0(None, model, [], torch.device("cpu"), 0, tracker="viterbi", tracker_options=dict(threshold=0.1))
    with pytest.raises(ValueError, match="tracker_options"):
        evaluate.test_conversion_f0(None, model, [], torch.device("cpu"), 0, tracker="yin", tracker_options=dict(jump_cost=0.1))
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.test_conversion_f0(None, model, [], torch.device("cpu"), 0, tracker="viterbi", tracker_options=dict(jump_cost=0.1))
