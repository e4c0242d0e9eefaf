"""CPU tests of fast Griffin-Lim and the spectral-convergence figure (include/nsg.h: nsg_audio_griffin_lim_fast,
nsg_audio_spectral_convergence): the fp64 restatement tests/helpers/griffin_lim_fast_ref.py against the oracle, the convergence
claim that tests/test_gpu_griffin_lim_fast.py relies on, what the entry points refuse before any launch (pointers that are never
dereferenced), and the spectral-convergence bound shown reachable by an fp32 restatement without any kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

from neural_sound_generation_amd import _lib
from oracle import audio_oracle as A
from tests.helpers import audio_envelope as E, griffin_lim_fast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL = 0x10000, 0
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p


def _refused(lib, name, rc, want):
    msg = lib.nsg_last_error_string()
    return rc == want and msg is not None and msg.startswith(name.encode() + b":")


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,T", R.GL_FAST_CASES)
def test_restatement_at_momentum_zero_is_the_oracle(n_fft, hop, T):
    """The two differ only in exp(i angle(X)) against X / |X|: a few 1e-15 of max|y| (2.4e-15 seen)."""
    S, u = E.gl_case(n_fft, hop, T, B=1)
    S, u = S[0].T.astype(np.float64), u[0].T.astype(np.float64)
    for iters in (0, 1, 3, 8):
        want = A.griffin_lim(S, n_fft, hop, iters, u)
        got, X = R.griffin_lim_fast(S, n_fft, hop, iters, u, 0.0, want_state=True)
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"{n_fft}/{hop} T={T} iters={iters}: {rel:.2e}")
        assert rel <= 1e-12
        assert (X is None) == (iters == 0)


def test_state_is_the_stft_of_the_last_but_one_waveform():
    S, u = E.gl_case(512, 128, 5, B=1)
    S, u = S[0].T.astype(np.float64), u[0].T.astype(np.float64)
    y2 = R.griffin_lim_fast(S, 512, 128, 2, u, 0.99)
    _, X3 = R.griffin_lim_fast(S, 512, 128, 3, u, 0.99, want_state=True)
    assert np.array_equal(X3, A.stft(y2, 512, 128))


def test_first_iteration_does_not_depend_on_the_momentum():
    """t_1 = (1 + momentum) X_1 has the phase of X_1: one iteration is the plain one whatever the momentum."""
    S, u = E.gl_case(512, 64, 9, B=1)
    S, u = S[0].T.astype(np.float64), u[0].T.astype(np.float64)
    y0 = R.griffin_lim_fast(S, 512, 64, 1, u, 0.0)
    for m in (0.5, 0.99, 1.0):
        assert np.abs(R.griffin_lim_fast(S, 512, 64, 1, u, m) - y0).max() <= 1e-13 * np.abs(y0).max()


# ----------------------------------------------------------------------------------------------------------------------
# the convergence claim
# ----------------------------------------------------------------------------------------------------------------------
def test_sixteen_fast_iterations_beat_sixty_plain_ones_in_fp64():
    """On the harmonic signal, in fp64: 16 iterations at momentum 0.99 reach a lower spectral convergence than 60 plain ones (0.141
    against 0.164 measured: the 14 % gap is the margin an fp32 run gets), and 60 at 0.99 a lower one still (0.079)."""
    _, S, u = R.harmonic_case()
    assert S.shape == (257, 64)
    n, h = R.HARM_NFFT, R.HARM_HOP
    plain60 = R.spectral_convergence(R.griffin_lim_fast(S, n, h, 60, u, 0.0), S, n, h)
    fast16 = R.spectral_convergence(R.griffin_lim_fast(S, n, h, 16, u, 0.99), S, n, h)
    fast60 = R.spectral_convergence(R.griffin_lim_fast(S, n, h, 60, u, 0.99), S, n, h)
    print(f"plain 60: {plain60:.4f}  0.99 x 16: {fast16:.4f}  0.99 x 60: {fast60:.4f}")
    assert fast16 < plain60 and fast60 < fast16
    assert fast16 <= 0.9 * plain60                    # the margin the GPU test's fp32 trajectories get
    assert abs(plain60 - 0.164) <= 0.002 and abs(fast16 - 0.141) <= 0.002 and abs(fast60 - 0.079) <= 0.002


# ----------------------------------------------------------------------------------------------------------------------
# the ABI
# ----------------------------------------------------------------------------------------------------------------------
QUERIES = """nsg_audio_griffin_lim_workspace_bytes nsg_audio_mix_noise_workspace_bytes nsg_audio_tempo_workspace_bytes
nsg_audio_trim_workspace_bytes nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes nsg_bn_relu_c1convt_workspace_bytes
nsg_bn_relu_conv1x1_workspace_bytes nsg_bn_workspace_bytes nsg_c1conv_bn_workspace_bytes nsg_clip_colsum_workspace_bytes
nsg_conv_workspace_bytes nsg_cross_entropy_masked_workspace_bytes nsg_cross_entropy_workspace_bytes nsg_dtw_workspace_bytes
nsg_f0_viterbi_workspace_bytes nsg_gated_colsum_workspace_bytes nsg_grad_sumsq_workspace_bytes nsg_index_add_sorted_workspace_bytes
nsg_index_add_workspace_bytes nsg_reduce_workspace_bytes nsg_vae_latent_workspace_bytes nsg_vq_bf16x3_workspace_bytes
nsg_vq_losses_indexed_bn_workspace_bytes nsg_vq_workspace_bytes""".split()


def test_the_declarations_reach_the_binding_and_the_library():
    lib = _lib.load()
    for name in ("nsg_audio_griffin_lim_fast", "nsg_audio_spectral_convergence"):
        assert name in _lib.HEADER_SYMBOLS and hasattr(lib, name)
    ret, args = _lib._SIGS["nsg_audio_griffin_lim_fast"]
    assert ret is ctypes.c_int32 and args == [P] * 4 + [ctypes.c_int32] * 5 + [ctypes.c_float, P, ctypes.c_size_t, P]
    ret, args = _lib._SIGS["nsg_audio_spectral_convergence"]
    assert ret is ctypes.c_int32 and args == [P] * 4 + [ctypes.c_int32] * 4 + [P]


def test_no_new_workspace_query():
    """The momentum state is an argument, not a workspace section: fast Griffin-Lim takes nsg_audio_griffin_lim's workspace, the
    convergence sums take none, and the header's size queries are the 24 there were."""
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    declared = set(re.findall(r"NSG_API\s+size_t\s+(nsg_\w+_workspace_bytes)\s*\(", text))
    assert declared == set(QUERIES) and len(QUERIES) == 24


def test_griffin_lim_fast_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    name = "nsg_audio_griffin_lim_fast"
    good = dict(S=OK, u=OK, y=OK, c=OK, B=2, T=24, n_fft=1024, hop=256, iters=3, momentum=0.99, ws=OK, ws_bytes=None)

    def gl(**change):
        a = dict(good, **change)
        nb = lib.nsg_audio_griffin_lim_workspace_bytes(max(a["B"], 1), max(a["T"], 1), 1024) if a["ws_bytes"] is None else a["ws_bytes"]
        return lib.nsg_audio_griffin_lim_fast(P(a["S"]), P(a["u"]), P(a["y"]), P(a["c"]), a["B"], a["T"], a["n_fft"], a["hop"], a["iters"],
                                              a["momentum"], P(a["ws"]), nb, None)

    need = lib.nsg_audio_griffin_lim_workspace_bytes(2, 24, 1024)
    for change in (dict(S=NULL), dict(u=NULL), dict(y=NULL), dict(B=0), dict(B=-1), dict(T=1), dict(T=0), dict(T=-3), dict(hop=0), dict(hop=-256),
                   dict(iters=-1), dict(momentum=-0.01), dict(momentum=1.01), dict(momentum=-1.0), dict(momentum=2.0),
                   dict(momentum=float("nan")), dict(momentum=float("inf")), dict(momentum=-float("inf")),
                   dict(c=NULL), dict(c=NULL, momentum=0.5), dict(c=NULL, momentum=1.0), dict(c=NULL, momentum=1e-30)):
        assert _refused(lib, name, gl(**change), INVALID), change
    # momentum and c are refused before the workspace is looked at, and before any launch
    for change in (dict(momentum=float("nan"), ws=NULL), dict(c=NULL, ws_bytes=0)):
        assert _refused(lib, name, gl(**change), INVALID), change
    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(n_fft=0), dict(hop=200), dict(hop=384), dict(hop=2048),
                   dict(hop=1, T=2),                                       # a one-sample grid: no reflection exists
                   dict(B=1 << 16, T=1 << 15, ws_bytes=1 << 62)):          # B * T = 2^31 frames
        assert _refused(lib, name, gl(**change), UNSUPPORTED), change
    for m in (0.99, 0.0, 1.0):
        for change in (dict(ws=NULL), dict(ws_bytes=0), dict(ws_bytes=need - 1), dict(ws_bytes=need // 2)):
            assert _refused(lib, name, gl(momentum=m, **change), WORKSPACE), (m, change)
            assert b"workspace too small" in lib.nsg_last_error_string()
    # momentum 0 needs no state buffer, and the smallest grids are refused for nothing but the workspace (the checks above it passed)
    for change in (dict(c=NULL, momentum=0.0), dict(hop=2, T=2), dict(hop=1, T=3), dict(hop=1024, T=2), dict(hop=128, T=2), dict(momentum=1.0),
                   dict(momentum=0.0)):
        assert _refused(lib, name, gl(ws=NULL, **change), WORKSPACE), change


def test_spectral_convergence_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    name = "nsg_audio_spectral_convergence"

    def sc(y=OK, S=OK, frames=OK, clips=OK, B=2, T=24, n_fft=1024, hop=256):
        return lib.nsg_audio_spectral_convergence(P(y), P(S), P(frames), P(clips), B, T, n_fft, hop, None)

    for change in (dict(y=NULL), dict(S=NULL), dict(clips=NULL), dict(clips=NULL, frames=NULL), dict(B=0), dict(B=-1), dict(T=1), dict(T=0), dict(hop=0),
                   dict(hop=-256)):
        assert _refused(lib, name, sc(**change), INVALID), change
    for change in (dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(hop=200), dict(hop=2048), dict(hop=1, T=2), dict(B=1 << 16, T=1 << 15)):
        assert _refused(lib, name, sc(**change), UNSUPPORTED), change


# ----------------------------------------------------------------------------------------------------------------------
# the spectral-convergence bound
# ----------------------------------------------------------------------------------------------------------------------
def _sc_inputs():
    """The GPU test's inputs: (tag, n_fft, hop, y float32, S float32 (F, T)): gl_case magnitudes with the fp64 fast Griffin-Lim output
    for them, and the band-limited signal with its own magnitudes."""
    for n_fft, hop, T in R.GL_FAST_CASES:
        S, u = E.gl_case(n_fft, hop, T, B=1)
        y = R.griffin_lim_fast(S[0].T.astype(np.float64), n_fft, hop, 3, u[0].T.astype(np.float64), 0.99)
        yield f"gl {n_fft}/{hop} T={T}", n_fft, hop, y.astype(np.float32), S[0].T
    for n_fft, hop, T in ((512, 128, 24), (1024, 256, 24), (2048, 512, 9)):
        y, S = R.band_limited_case(n_fft, hop, T)
        yield f"band-limited {n_fft}/{hop} T={T}", n_fft, hop, y, S


def test_an_fp32_restatement_lies_within_the_spectral_convergence_bound():
    """|sc_32 - sc_64| <= eps (1 + sc_64), eps = (2 log2 N + 8) 2^-24 (R.sc_eps: the derivation), for a numpy / torch restatement in
    fp32 with a complex64 FFT: the bound is reachable without any kernel.  Measured share of the bound: 0.001 or less on five of
    the six gl cases, 0.18 at hop == n_fft (1024/1024 T=4), 0.05 on the three band-limited signals."""
    for tag, n_fft, hop, y, S in _sc_inputs():
        s64 = R.convergence_sums(y.astype(np.float64), S.astype(np.float64), n_fft, hop)
        s32 = R.convergence_sums_c64(y, S, n_fft, hop)
        sc64, sc32 = float(R.figure(s64.sum(0))), float(R.figure(s32.sum(0)))
        bound = R.sc_eps(n_fft) * (1.0 + sc64)
        print(f"[{tag}] sc64={sc64:.3e} sc32={sc32:.3e} |diff|={abs(sc32 - sc64):.2e} bound={bound:.2e} share={abs(sc32 - sc64) / bound:.3f}")
        assert abs(sc32 - sc64) <= bound, tag
        assert np.array_equal(s32[:, 1], s64[:, 1])                       # S is the same fp32 array on both sides
        if tag.startswith("band"):
            assert sc64 <= E.U32 and sc32 <= R.sc_eps(n_fft)


def test_sc_eps_is_the_stated_formula():
    for n_fft, lg in ((512, 9), (1024, 10), (2048, 11)):
        assert R.sc_eps(n_fft) == (2 * lg + 8) * 2.0 ** -24


def test_figure_of_zero_sums():
    assert R.figure(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 4.0], [0.0, 4.0]])).tolist() == [0.0, float("inf"), 0.5, 0.0]


def test_python_refuses_a_bad_momentum_before_anything_is_launched():
    import torch
    from neural_sound_generation_amd import audio, evaluate, models
    for m in (-0.1, 1.5, float("nan"), "0.5", True, None):
        with pytest.raises(ValueError, match="momentum"):
            audio._momentum("griffin_lim", m)
        with pytest.raises(ValueError, match="momentum"):
            evaluate.test_conversion_f0(None, models.VQVAE(1, 16, 32, n_speakers=2), [], torch.device("cpu"), 0, momentum=m)
    assert audio._momentum("griffin_lim", 1) == 1.0 and audio._momentum("griffin_lim", np.float32(0.5)) == 0.5
    assert audio._momentum("griffin_lim", 1e-50) == 0.0 and audio._momentum("griffin_lim", 0.99) == float(np.float32(0.99))      # as the kernel gets it
