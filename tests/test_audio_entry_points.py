"""CPU tests of the mel -> waveform entry points of csrc/audio.hip: what they refuse before any launch (pointers that are
never dereferenced, as in tests/test_preprocess.py), the reflect map of stft_frame_lds restated in Python against
np.pad(mode="reflect"), and what the derived bounds of tests/helpers/audio_envelope.py assume about their inputs."""
import ctypes

import numpy as np
import pytest

from neural_sound_generation_amd import _lib
from tests.helpers import audio_envelope as E

OK, NULL = 0x10000, 0
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p


def _refused(lib, name, rc, want):
    msg = lib.nsg_last_error_string()
    return rc == want and msg is not None and msg.startswith(name.encode() + b":")


# ----------------------------------------------------------------------------------------------------------------------
# the reflect map
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", E.REFLECT_TABLE)
def test_reflect_map_is_numpys_for_every_short_grid(n_fft, hop):
    """The kernel's index arithmetic (C remainder included) against np.pad(np.arange(L), n_fft/2, "reflect") at every padded
    position, L = hop (T - 1) for T in 2..12: from grids a quarter (an eighth at hop = n_fft/8) of the padding up to grids
    longer than it."""
    for T in range(2, 13):
        L = hop * (T - 1)
        want = np.pad(np.arange(L), n_fft // 2, mode="reflect")
        got = np.array([E.reflect_index_fixed(i - n_fft // 2, L) for i in range(L + n_fft)])
        assert np.array_equal(got, want), (n_fft, hop, T, int((got != want).sum()))


def test_reflect_map_small_and_odd_lengths():
    """Every L in 2..40 (odd ones and L = 2, whose period is 2, included) under a padding of 64 and of 1024."""
    for L in range(2, 41):
        for pad in (64, 1024):
            want = np.pad(np.arange(L), pad, mode="reflect")
            got = np.array([E.reflect_index_fixed(i - pad, L) for i in range(L + 2 * pad)])
            assert np.array_equal(got, want), (L, pad)


def test_one_fold_map_is_exact_only_above_half_a_window():
    """The precondition melspectrogram_kernel states: for L > n_fft/2 one fold is numpy's map; the counts of wrong positions
    for shorter grids are the ones that made Griffin-Lim wrong on short clips (1024/256: 259 at T = 2, the right edge at 3)."""
    for n_fft in (512, 1024, 2048):
        for L in (n_fft // 2 + 1, n_fft // 2 + 2, n_fft, 3 * n_fft + 7):
            want = np.pad(np.arange(L), n_fft // 2, mode="reflect")
            got = np.array([E.reflect_index_one_fold(i - n_fft // 2, L) for i in range(L + n_fft)])
            assert np.array_equal(got, want), (n_fft, L)

    def wrong(n_fft, hop, T):
        L = hop * (T - 1)
        want = np.pad(np.arange(L), n_fft // 2, mode="reflect")
        return int(sum(E.reflect_index_one_fold(i - n_fft // 2, L) != want[i] for i in range(L + n_fft)))
    assert [wrong(1024, 256, T) for T in (2, 3, 4)] == [259, 1, 0]
    assert [wrong(1024, 128, T) for T in (2, 3, 4, 5, 6)] == [641, 259, 129, 1, 0]
    assert [wrong(1024, 512, T) for T in (2, 3)] == [1, 0]
    assert wrong(1024, 1024, 2) == 0


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_griffin_lim_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    name = "nsg_audio_griffin_lim"
    good = dict(S=OK, u=OK, y=OK, B=2, T=24, n_fft=1024, hop=256, iters=3, ws=OK, ws_bytes=None)

    def gl(**change):
        a = dict(good, **change)
        nb = lib.nsg_audio_griffin_lim_workspace_bytes(max(a["B"], 1), max(a["T"], 1), 1024) if a["ws_bytes"] is None else a["ws_bytes"]
        return lib.nsg_audio_griffin_lim(P(a["S"]), P(a["u"]), P(a["y"]), a["B"], a["T"], a["n_fft"], a["hop"], a["iters"], P(a["ws"]), nb, None)

    need = lib.nsg_audio_griffin_lim_workspace_bytes(2, 24, 1024)
    for change in (dict(S=NULL), dict(u=NULL), dict(y=NULL), dict(B=0), dict(B=-1), dict(T=1), dict(T=0), dict(T=-3), dict(hop=0), dict(hop=-256),
                   dict(iters=-1)):
        assert _refused(lib, name, gl(**change), INVALID), change
    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(n_fft=0), dict(hop=200), dict(hop=384), dict(hop=2048),
                   dict(hop=1, T=2),                                       # a one-sample grid: no reflection exists
                   dict(B=1 << 16, T=1 << 15, ws_bytes=1 << 62)):          # B * T = 2^31 frames
        assert _refused(lib, name, gl(**change), UNSUPPORTED), change
    for change in (dict(ws=NULL), dict(ws_bytes=0), dict(ws_bytes=need - 1), dict(ws_bytes=need // 2)):
        assert _refused(lib, name, gl(**change), WORKSPACE), change
    # the smallest grids the entry point accepts are refused for nothing but the workspace here (so the checks above it passed)
    for change in (dict(hop=2, T=2), dict(hop=1, T=3), dict(hop=1024, T=2), dict(hop=128, T=2)):
        assert _refused(lib, name, gl(ws=NULL, **change), WORKSPACE), change


def _grid_entry_points(lib):
    """name -> (call(B, T, n_fft, hop, ws, ws_bytes), takes a workspace) for the four entry points on Griffin-Lim's grid, every
    other argument good."""
    return {
        "nsg_audio_griffin_lim":
            (lambda B, T, n, h, ws, nb: lib.nsg_audio_griffin_lim(P(OK), P(OK), P(OK), B, T, n, h, 3, P(ws), nb, None), True),
        "nsg_audio_griffin_lim_fast":
            (lambda B, T, n, h, ws, nb: lib.nsg_audio_griffin_lim_fast(P(OK), P(OK), P(OK), P(OK), B, T, n, h, 3, 0.99, P(ws), nb, None), True),
        "nsg_audio_spsi_phases":
            (lambda B, T, n, h, ws, nb: lib.nsg_audio_spsi_phases(P(OK), P(OK), B, T, n, h, P(ws), nb, None), True),
        "nsg_audio_spectral_convergence":
            (lambda B, T, n, h, ws, nb: lib.nsg_audio_spectral_convergence(P(OK), P(OK), P(OK), P(OK), B, T, n, h, None), False),
    }


@pytest.mark.parametrize("name", ["nsg_audio_griffin_lim", "nsg_audio_griffin_lim_fast", "nsg_audio_spsi_phases", "nsg_audio_spectral_convergence"])
def test_the_four_entry_points_on_griffin_lims_grid_refuse_the_same_grids(name):
    """The bad grids of test_griffin_lim_refuses_bad_arguments_before_any_launch, fed to every entry point that takes that grid:
    the same code, under the entry point's own name, with a workspace that would do (so the grid alone is refused) and with none
    (the grid is judged before the workspace).  The two stated differences: SPSI takes a single frame and the one-sample grid,
    which it reflects nowhere, as far as its workspace check."""
    lib = _lib.load()
    call, has_ws = _grid_entry_points(lib)[name]
    good = dict(B=2, T=24, n_fft=1024, hop=256)
    spsi = name == "nsg_audio_spsi_phases"

    def run(ws=OK, ws_bytes=1 << 62, **change):
        a = dict(good, **change)
        return call(a["B"], a["T"], a["n_fft"], a["hop"], ws, ws_bytes)

    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(n_fft=0), dict(hop=200), dict(hop=384), dict(hop=2048),
                   dict(B=1 << 16, T=1 << 15)):                            # B * T = 2^31 frames
        assert _refused(lib, name, run(**change), UNSUPPORTED), change
        assert _refused(lib, name, run(ws=NULL, ws_bytes=0, **change), UNSUPPORTED), change
    assert b"too many frames" in lib.nsg_last_error_string()
    # a one-sample grid has no reflection, a single frame no samples at all: only SPSI, which forms no frame of samples, takes them
    assert _refused(lib, name, run(ws=NULL, hop=1, T=2), WORKSPACE if spsi else UNSUPPORTED)
    assert _refused(lib, name, run(ws=NULL, T=1), WORKSPACE if spsi else INVALID)
    if has_ws:
        need = lib.nsg_audio_griffin_lim_workspace_bytes(2, 24, 1024)
        for ws, nb in ((NULL, need), (OK, need - 1), (OK, 0)):
            assert _refused(lib, name, run(ws=ws, ws_bytes=nb), WORKSPACE), (ws, nb)
            assert b"workspace too small" in lib.nsg_last_error_string()


def test_griffin_lim_workspace_bytes():
    lib = _lib.load()
    q = lib.nsg_audio_griffin_lim_workspace_bytes
    for args in ((0, 24, 1024), (2, 0, 1024), (2, 24, 0), (-1, 24, 1024), (2, -24, 1024), (2, 24, -1024)):
        assert q(*args) == 0, args
    for B, T, n_fft in ((1, 2, 512), (2, 24, 1024), (3, 5, 2048), (64, 1024, 1024)):
        spec = B * T * (n_fft // 2 + 1) * 2 * 4           # complex spectra [B][T][F]
        frames = B * T * n_fft * 4                        # windowed inverse transforms [B][T][n_fft]
        assert q(B, T, n_fft) >= spec + frames, (B, T, n_fft)
        assert q(B, T, n_fft) <= spec + frames + 512      # two 256-byte roundings, nothing else


def test_stft_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    name = "nsg_audio_stft"

    def stft(y=OK, X=OK, B=2, L=4096, n_fft=1024, hop=256):
        return lib.nsg_audio_stft(P(y), P(X), B, L, n_fft, hop, None)

    for change in (dict(y=NULL), dict(X=NULL), dict(B=0), dict(L=0), dict(L=-7), dict(hop=0), dict(hop=-1)):
        assert _refused(lib, name, stft(**change), INVALID), change
    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096),
                   dict(L=512), dict(L=1), dict(L=511), dict(n_fft=2048, L=1024), dict(n_fft=512, L=256),      # L <= n_fft / 2
                   dict(B=1 << 20, L=1 << 20, hop=1),                                                         # B * T about 2^40
                   dict(B=1 << 15, L=(1 << 16) - 1, hop=1)):                                                  # B * T = 2^31 exactly
        assert _refused(lib, name, stft(**change), UNSUPPORTED), change
    assert b"too many frames" in lib.nsg_last_error_string()


def test_inv_preemphasis_and_mel_to_linear_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    name = "nsg_audio_inv_preemphasis"
    for args in ((P(NULL), P(OK + 64), 1, 8), (P(OK), P(NULL), 1, 8), (P(OK), P(OK), 1, 8),                   # null, in place
                 (P(OK), P(OK + 64), 0, 8), (P(OK), P(OK + 64), 1, 0)):
        assert _refused(lib, name, lib.nsg_audio_inv_preemphasis(*args, 0.97, None), INVALID), args
    for k in (1.0, -1.0, 1.5, -2.0, float("inf")):
        assert _refused(lib, name, lib.nsg_audio_inv_preemphasis(P(OK), P(OK + 64), 1, 8, k, None), UNSUPPORTED), k
    assert lib.nsg_audio_inv_preemphasis(P(OK), P(OK + 64), 1, 8, float("nan"), None) != 0                    # never launched with a nan k
    assert _refused(lib, "nsg_audio_preemphasis", lib.nsg_audio_preemphasis(P(OK), P(OK), 1, 8, 0.97, None), INVALID)

    name = "nsg_audio_mel_to_linear"

    def m2l(mel=OK, inv=OK, S=OK, B=2, n_mels=80, T=11, F=513, max_abs=1.0):
        return lib.nsg_audio_mel_to_linear(P(mel), P(inv), P(S), B, n_mels, T, F, -100.0, 20.0, max_abs, 1.5, None)

    for change in (dict(mel=NULL), dict(inv=NULL), dict(S=NULL), dict(B=0), dict(n_mels=0), dict(T=0), dict(F=0), dict(max_abs=0.0),
                   dict(max_abs=-1.0)):
        assert _refused(lib, name, m2l(**change), INVALID), change
    for change in (dict(B=1 << 16, T=1 << 15), dict(B=1 << 20, T=1 << 20), dict(B=1, T=0x7fffffff)):           # B * T >= 2^31 - 1
        assert _refused(lib, name, m2l(**change), UNSUPPORTED), change


# ----------------------------------------------------------------------------------------------------------------------
# what the derived bounds assume about their inputs (oracle only)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [40, 80])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_mel_to_linear_inputs_stay_inside_the_clamp_cap(n_mels, n_fft):
    """The interval test of mel_to_linear excuses an entry whose fp64 sum lies within its error bound of the clamp at 1e-10.
    That rule must stay an exception: at most 1 % of the entries of any case, none with a sum above 1e-8; and the inputs
    must hold what they are there for (exact 0 and 1, values outside [0, 1], clamped and unclamped outputs)."""
    for T in (1, 11, 257):
        mel = E.m2l_input(n_mels, T, E.m2l_seed(n_mels, n_fft, T))
        if T > 1:
            assert (mel == 0).any() and (mel == 1).any() and (mel < 0).any() and (mel > 1).any()
        for b in range(mel.shape[0]):
            S64, lo, hi, straddles, acc = E.m2l_bounds(mel[b], 22050, n_fft, n_mels)
            assert straddles.mean() <= E.M2L_CLAMP_CAP, (T, b, straddles.mean())
            assert not (straddles & (acc > 1e-8)).any(), (T, b, acc[straddles & (acc > 1e-8)])
            clamped = (acc <= E.CLAMP).mean()
            assert 0.1 < clamped < 0.9, (T, b, clamped)                  # both sides of the clamp are exercised
            assert (lo <= S64).all() and (S64 <= hi).all() and (lo > 0).all()


def test_inv_preemphasis_bound_is_rounding_sized():
    """The bound handed to the kernel is 4 x the fp32 recurrence's own error + 1e-9 max|y|.  It must stay a rounding-sized
    number: relative to max|y| it is below 1e-4 everywhere (k = 0.999 on a constant, gain 1000, is the largest at 7e-5;
    k = 0.97 on noise 1e-6), and for k = 0 the filter is the identity, so the fp32 error is exactly zero."""
    worst = 0.0
    for L in E.PRE_LENGTHS:
        for k in E.PRE_KS:
            for name, x in E.pre_inputs(L).items():
                y64, bound, e32 = E.pre_bound(x, k)
                if k == 0.0:
                    assert e32 == 0.0
                peak = np.abs(y64).max()
                if peak == 0.0:                                          # (the slow sine at L = 1 is the sample 0)
                    assert bound == 0.0
                else:
                    worst = max(worst, bound / peak)
    assert worst < 1e-4, worst
