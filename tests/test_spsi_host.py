"""CPU tests of the single-pass spectrogram inversion phases (include/nsg.h: nsg_audio_spsi_phases): properties of the fp64
restatement tests/helpers/spsi_ref.py, the declaration's way into the binding and the library, what the entry point and the Python
wrappers refuse before any launch (pointers that are never dereferenced), the workspace layout against Griffin-Lim's query, and the
convergence claim that tests/test_gpu_spsi.py relies on."""
import ctypes
import os
import re

import numpy as np
import pytest

from neural_sound_generation_amd import _lib
from oracle import audio_oracle as A
from tests.helpers import spsi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL = 0x10000, 0
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p
NAME = "nsg_audio_spsi_phases"


def _refused(lib, rc, want):
    msg = lib.nsg_last_error_string()
    return rc == want and msg is not None and msg.startswith(NAME.encode() + b":")


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,j", [(512, 128, 37), (1024, 256, 100), (1024, 1024, 3), (2048, 32, 1000)])
def test_a_tone_at_a_bin_centre_has_no_offset_and_advances_at_its_bin(n_fft, hop, j):
    """The true Hann magnitudes of cos(2 pi j n / n_fft): the lobe is (1/2, 1, 1/2) A around bin j, symmetric, so p == 0 exactly
    once a == c in fp32; the peak's phase then advances by hop j / n_fft turns a frame, mod 1, exactly."""
    T = 7
    n = np.arange(hop * (T - 1) + n_fft)
    S = np.abs(A.stft(np.cos(2 * np.pi * j * n / n_fft)[:max(hop * (T - 1), n_fft)], n_fft, hop)).astype(np.float32).T
    S = S[1:-1] if len(S) > 4 else S                              # away from the reflected ends
    m = S[len(S) // 2].copy()
    m[j - 1] = m[j + 1]                                           # the two sides agree to rounding; make them agree in fp32
    assert j in R.peaks_of(m)
    assert R.peak_offsets(m, np.array([j]))[0] == 0.0
    frames = np.tile(m, (5, 1))
    _, phi = R.spsi_phases(frames, n_fft, hop, want_state=True)
    for t in range(5):
        assert phi[t, j] == ((t + 1) * hop * j / n_fft) % 1.0
    assert (phi[:, j - 1] == phi[:, j]).all() and (phi[:, j + 1] == phi[:, j]).all()      # the lobe is locked to its peak


def test_a_plateau_is_no_peak_and_a_nan_is_never_one():
    m = np.array([0, 1, 2, 2, 1, 0, 3, 0, np.nan, 0, 5, np.nan, 0], dtype=np.float32)
    assert R.peaks_of(m).tolist() == [6]


def test_the_first_minimum_decides_a_tie():
    m = np.array([0, 9, 4, 2, 2, 4, 8, 1, 1, 7, 0, 0], dtype=np.float32)
    pk = R.peaks_of(m)
    assert pk.tolist() == [1, 6, 9]
    # m[1 .. 6] = 9 4 2 2 4 8: the minimum 2 is first at bin 3; m[6 .. 9] = 8 1 1 7: first at bin 7
    assert R.owners(m, pk).tolist() == [1, 1, 1, 1, 6, 6, 6, 6, 9, 9, 9, 9]


@pytest.mark.parametrize("value", [0.0, 0.75])
def test_a_frame_without_a_peak_advances_at_bin_centres(value):
    n_fft, hop, T = 512, 128, 6
    F = n_fft // 2 + 1
    ang, phi = R.spsi_phases(np.full((T, F), value, np.float32), n_fft, hop, want_state=True)
    k = np.arange(F)
    for t in range(T):
        assert np.array_equal(phi[t], ((t + 1) * k * hop / n_fft) % 1.0)
        assert np.array_equal(ang[t], ((phi[t] + 0.5 * k) % 1.0).astype(np.float32))
    assert ang.min() >= 0.0 and ang.max() < 1.0


def test_the_offset_is_inside_half_a_bin_and_the_angles_inside_a_turn():
    S = R.patterns(512, 33, 1)["random"][0]
    for m in S[:4]:
        pk = R.peaks_of(m)
        assert len(pk) and (np.abs(R.peak_offsets(m, pk)) < 0.5).all()
    ang = R.spsi_phases(S, 512, 32)
    assert ang.dtype == np.float32 and ang.min() >= 0.0 and ang.max() < 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_the_declaration_reaches_the_binding_and_the_library():
    lib = _lib.load()
    assert NAME in _lib.HEADER_SYMBOLS and hasattr(lib, NAME)
    ret, args = _lib._SIGS[NAME]
    assert ret is ctypes.c_int32 and args == [P, P] + [ctypes.c_int32] * 4 + [P, ctypes.c_size_t, P]


def test_no_workspace_query_of_its_own():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    declared = set(re.findall(r"NSG_API\s+size_t\s+(nsg_\w+_workspace_bytes)\s*\(", text))
    assert len(declared) == 24 and not any("spsi" in q for q in declared)


def _call(lib, **change):
    a = dict(dict(S=OK, angles=OK, B=2, T=24, n_fft=1024, hop=256, ws=OK, ws_bytes=None), **change)
    nb = lib.nsg_audio_griffin_lim_workspace_bytes(max(a["B"], 1), max(a["T"], 1), 1024) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.nsg_audio_spsi_phases(P(a["S"]), P(a["angles"]), a["B"], a["T"], a["n_fft"], a["hop"], P(a["ws"]), nb, None)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    for change in (dict(S=NULL), dict(angles=NULL), dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(hop=0), dict(hop=-256),
                   dict(S=NULL, ws=NULL), dict(T=0, ws_bytes=0)):
        assert _refused(lib, _call(lib, **change), INVALID), change
    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(n_fft=0), dict(hop=200), dict(hop=384), dict(hop=2048),
                   dict(B=1 << 16, T=1 << 15, ws_bytes=1 << 62),           # B * T = 2^31 frames
                   dict(n_fft=1000, ws=NULL)):
        assert _refused(lib, _call(lib, **change), UNSUPPORTED), change
    need = lib.nsg_audio_griffin_lim_workspace_bytes(2, 24, 1024)
    for change in (dict(ws=NULL), dict(ws_bytes=0), dict(ws_bytes=need - 1), dict(ws_bytes=need // 2)):
        assert _refused(lib, _call(lib, **change), WORKSPACE), change
        assert b"workspace too small" in lib.nsg_last_error_string()
    # a single frame, and the grids Griffin-Lim refuses as too short, are refused for nothing but the workspace
    for change in (dict(T=1), dict(T=1, hop=1024), dict(T=2, hop=1), dict(B=1, T=1, n_fft=512, hop=32), dict(n_fft=2048, hop=2048, T=3)):
        assert _refused(lib, _call(lib, ws=NULL, **change), WORKSPACE), change


def test_the_layout_fits_the_griffin_lim_query_over_the_envelope():
    """csrc/audio.hip's spsi_layout: the advances [B][T][F] fp64 | the owners [B][T][F] uint16, each section rounded up to 256 bytes."""
    lib = _lib.load()

    def up(n):
        return -(-n // 256) * 256

    for n_fft in R.NFFTS:
        F = n_fft // 2 + 1
        for B in (1, 2, 3, 64, 1000):
            for T in (1, 2, 3, 33, 862, 100003):
                have = lib.nsg_audio_griffin_lim_workspace_bytes(B, T, n_fft)
                assert up(B * T * F * 8) + up(B * T * F * 2) <= have, (n_fft, B, T)
                assert have >= (16 * F - 8) * B * T                    # Griffin-Lim's: 8 F for the spectrum and 4 n_fft = 8 F - 8 for the frame


def test_python_refuses_bad_arguments_before_anything_is_launched():
    import torch
    from neural_sound_generation_amd import audio, evaluate, models
    S = torch.zeros(1, 3, 513)
    for kw in (dict(fft_size=1000), dict(fft_size=True), dict(hop_size=0), dict(hop_size=384), dict(hop_size=2.0), dict(fft_size=512)):
        with pytest.raises(ValueError, match="spsi_phases"):
            audio.spsi_phases(S, **kw)
    for bad in (torch.zeros(3, 513), torch.zeros(1, 0, 513), np.zeros((1, 3, 513), np.float32)):
        with pytest.raises(ValueError, match="spsi_phases"):
            audio.spsi_phases(bad)
    with pytest.raises(_lib.NsgError, match="GPU tensor"):
        audio.spsi_phases(S)
    mel = np.zeros((80, 8), np.float32)
    for init in ("SPSI", "zeros", None, 1):
        with pytest.raises(ValueError, match="init"):
            audio.inv_mel_spectrogram(mel, init=init)
        with pytest.raises(ValueError, match="init"):
            evaluate.test_conversion_f0(None, models.VQVAE(1, 16, 32, n_speakers=2), [], torch.device("cpu"), 0, init=init)
        with pytest.raises(ValueError, match="init"):
            evaluate.continue_audio(None, None, None, None, 0, 8, init=init)
    a0 = np.zeros((1, 8, 513), np.float32)
    with pytest.raises(ValueError, match="angles0"):
        audio.inv_mel_spectrogram(mel, init="spsi", angles0=a0)
    with pytest.raises(ValueError, match="angles0"):
        evaluate.test_conversion_f0(None, models.VQVAE(1, 16, 32, n_speakers=2), [], torch.device("cpu"), 0, init="spsi", angles0=a0)
    with pytest.raises(ValueError, match="angles0"):
        evaluate.continue_audio(None, None, None, None, 0, 8, init="spsi", angles0=a0)
    assert audio._init("f", "random", a0) == "random" and audio._init("f", "spsi", None) == "spsi"


# ----------------------------------------------------------------------------------------------------------------------
# the convergence claim
# ----------------------------------------------------------------------------------------------------------------------
def test_two_cells_of_the_trial_table_are_reproduced():
    """n_fft 1024, hop 256, 120 frames, a gliding 29-harmonic tone, true magnitudes, 0 iterations: the write-up's table says 0.640 from
    random phases and 0.152 from SPSI phases.  The signal here is built to that description, not the trial's own samples, so the band
    is loose: the random cell, which depends on the window and the overlap alone, within 5 %; the SPSI cell, which depends on how
    fast the tone glides, within a factor 1.5 either way.  Measured here: 0.648 and 0.200."""
    S, u = R.trial_case(**R.TRIAL)
    n, h = R.TRIAL["n_fft"], R.TRIAL["hop"]
    assert S.shape == (513, 120)
    rand0 = R.convergence_from(S, n, h, u, 0)
    spsi0 = R.convergence_from(S, n, h, R.spsi_phases(S.T, n, h).T.astype(np.float64), 0)
    print(f"random {rand0:.4f}  spsi {spsi0:.4f}")
    assert abs(rand0 - 0.640) <= 0.05 * 0.640
    assert 0.152 / 1.5 <= spsi0 <= 0.152 * 1.5


def test_the_relations_the_gpu_test_asserts_hold_in_fp64():
    """On the GPU test's signal (n_fft 512, hop 128, 60 frames), in fp64: from SPSI phases the spectral convergence after 0 and after 4
    plain iterations is below the same from random phases, and at 0 iterations below half of it.  Measured: 0.092 against 0.638
    (ratio 0.14) and 0.064 against 0.289: the margins an fp32 run gets."""
    S, u = R.trial_case(**R.POINT)
    n, h = R.POINT["n_fft"], R.POINT["hop"]
    a = R.spsi_phases(S.T, n, h).T.astype(np.float64)
    r0, r4 = (R.convergence_from(S, n, h, u, i) for i in (0, 4))
    s0, s4 = (R.convergence_from(S, n, h, a, i) for i in (0, 4))
    print(f"random {r0:.4f} {r4:.4f}  spsi {s0:.4f} {s4:.4f}")
    assert s0 < 0.5 * r0 and s4 < r4 and s0 < r0
    assert s0 <= 0.25 * r0 and s4 <= 0.5 * r4              # the margin
