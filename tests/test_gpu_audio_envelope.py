"""GPU tests of the mel -> waveform kernels (csrc/audio.hip) across their envelope: all three FFT sizes, hops from n_fft/8 to
n_fft, grids shorter than the reflect padding, a production-sized batch, degenerate magnitudes, chunk-boundary lengths.

Every comparison is against the fp64 restatement oracle/audio_oracle.py or an exact identity; a second run of the code under
test is the reference only where bit-equality is the property (batch independence, determinism, the wrapper's composition).
Every tolerance is computed here from the oracle and the precision of fp32 (tests/helpers/audio_envelope.py holds the
derivations); the kernels' measured errors are recorded beside them.  Each test prints its figures before it asserts.

NOT YET MEASURED ON AN MI355X: the kernels' errors that belong beside each bound below (each test prints them before it
asserts) have not been recorded; the figures quoted are those of the oracle and of a numpy fp32 restatement on the CPU.
Griffin-Lim: the oracle's response to a 2^-24 perturbation of S, as a fraction of max|y| over the 90 clip-cases per
iteration count, is 5.0e-8 .. 1.7e-7 (median 7.3e-8) at 0 iterations, 4.7e-8 .. 7.9e-6 (median 1.4e-7) at 1 and
4.8e-8 .. 7.1e-6 (median 1.5e-7) at 3; the allowed multiple is 512 (E.GL_MULTIPLE).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import audio as Au  # noqa: E402
from oracle import audio_oracle as A  # noqa: E402
from tests.helpers import audio_envelope as E, mel_forward64 as H  # noqa: E402

DEV = "cuda:0"
GL_GRIDS = [(512, 128), (1024, 256), (2048, 512), (1024, 128), (1024, 512), (512, 512)]
GL_FRAMES = [2, 3, 4, 5, 24]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# Griffin-Lim against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def check_griffin_lim(S, u, n_fft, hop, iters_list, tag, seeds=E.GL_SEEDS):
    """S, u (B, T, F) float32.  For every iteration count and clip: |y_gpu - y_oracle| <= 512 x (the oracle's largest response
    to a relative 2^-24 perturbation of S) x max|y_oracle| (E.GL_MULTIPLE: why 512).  Prints every figure, then asserts."""
    B, T, F = S.shape
    Sd, ud = dev(S), dev(u)
    rows = []
    for iters in iters_list:
        y = Au.griffin_lim(Sd, n_fft, hop, iters, ud).cpu().numpy()
        assert y.shape == (B, hop * (T - 1)) and np.isfinite(y).all(), (tag, iters)
        for b in range(B):
            want, resp = E.gl_response(S[b].T.astype(np.float64), n_fft, hop, iters, u[b].T.astype(np.float64), seeds=seeds)
            peak = float(np.abs(want).max())
            err = float(np.abs(y[b] - want).max())
            rows.append((iters, b, err, peak, resp))
            rel = err / peak if peak else 0.0
            print(f"[{tag}] iters={iters} clip={b}: err/max|y|={rel:.3e} response={resp:.3e} ratio={rel / resp if resp else 0.0:.1f} "
                  f"(allowed {E.GL_MULTIPLE:.0f}) max|y|={peak:.3e}")
    for iters, b, err, peak, resp in rows:
        assert err <= E.GL_MULTIPLE * resp * peak, (tag, iters, b, err / max(peak, 1e-300), resp)
    return rows


@pytest.mark.parametrize("T", GL_FRAMES)
@pytest.mark.parametrize("n_fft,hop", GL_GRIDS)
def test_griffin_lim_matches_the_oracle(n_fft, hop, T):
    """0, 1 and 3 iterations from the same phases, B = 3.  T = 2..5 are grids of hop (T - 1) samples, shorter than the n_fft/2
    of reflect padding whenever hop (T - 1) < n_fft/2: numpy's reflect map folds them more than once, and from the first
    iteration on the kernel must read the same samples.  hop == n_fft leaves the window's sum of squares at exactly zero at
    the frame joins (the `wss > tiny` branch) and at one tiny term beside them (the window must be accurate there)."""
    S, u = E.gl_case(n_fft, hop, T)
    check_griffin_lim(S, u, n_fft, hop, (0, 1, 3), f"gl {n_fft}/{hop} T={T}")


def test_griffin_lim_production_size():
    """B = 4 clips of T = 1024 frames at 1024/256 (what the epoch loop exports), 3 iterations."""
    S, u = E.gl_case(1024, 256, 1024, B=4)
    check_griffin_lim(S, u, 1024, 256, (3,), "gl production 4x1024", seeds=4)


@pytest.mark.parametrize("n_fft,T", [(1024, 24), (512, 5), (2048, 6)])
def test_griffin_lim_degenerate_magnitudes(n_fft, T):
    """All-zero frames, all-zero bins (DC, Nyquist and a band) and an all-zero clip: finite, within the same bound, and the
    all-zero clip exactly zero (its spectrum is exactly zero from the first iteration on: the np.angle(0) = 0 branch)."""
    S, u = E.degenerate_case(n_fft, T)
    check_griffin_lim(S[:2], u[:2], n_fft, n_fft // 4, (0, 1, 3), f"gl degenerate {n_fft} T={T}")
    for iters in (0, 1, 3):
        y = Au.griffin_lim(dev(S), n_fft, n_fft // 4, iters, dev(u))
        assert torch.isfinite(y).all()
        assert (y[2] == 0).all(), (iters, float(y[2].abs().max()))
        zero_alone = Au.griffin_lim(dev(S[2:]), n_fft, n_fft // 4, iters, dev(u[2:]))
        assert (zero_alone == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# perfect reconstruction: istft(stft(y)) == y
# ----------------------------------------------------------------------------------------------------------------------
# measured |y' - y| (max|y| 0.98 .. 1.0), against E.pr_tolerance = 1.34 (2 log2 N + 10.2) 2^-24:
# (kernels unmeasured; the numpy fp32 restatement gives 2.4e-7 .. 3.0e-7 against tolerances of 2.25e-6 / 2.41e-6 / 2.57e-6)
@pytest.mark.parametrize("n_fft,div", [(512, 4), (512, 8), (1024, 4), (1024, 8), (2048, 4), (2048, 8)])
def test_istft_of_stft_is_the_identity(n_fft, div):
    """The kernels' own transform pair: X = stft(y), then Griffin-Lim with 0 iterations from |X| and the phases of X is
    istft(X), which must return y on its hop (T - 1) samples.  Tolerance: E.pr_tolerance (the roundings of the two FFTs, the
    magnitude, the phase's trip through u = angle / 2 pi in fp32, the windows and the quotient)."""
    hop, T = n_fft // div, 40
    L = hop * (T - 1)
    y = E.pr_signal(L)
    X = Au.stft(dev(y[None]), n_fft, hop).cpu().numpy().astype(np.complex128)                 # (1, T, F)
    assert X.shape == (1, T, n_fft // 2 + 1)
    mag = np.abs(X).astype(np.float32)
    u = ((np.angle(X) / (2 * np.pi)) % 1.0).astype(np.float32)
    back = Au.griffin_lim(dev(mag), n_fft, hop, 0, dev(u)).cpu().numpy()[0]
    err, tol = float(np.abs(back - y).max()), E.pr_tolerance(n_fft)
    print(f"[pr {n_fft}/{hop}] max|istft(stft(y)) - y| = {err:.3e}  tolerance {tol:.3e}  max|y| = {np.abs(y).max():.4f}")
    assert back.shape == y.shape
    assert err <= tol, (err, tol)


# ----------------------------------------------------------------------------------------------------------------------
# batch independence and determinism (bit-equality IS the property)
# ----------------------------------------------------------------------------------------------------------------------
def test_a_clip_in_a_batch_is_the_clip_alone_and_runs_repeat():
    B = 5
    for n_fft, hop, T, iters in ((1024, 256, 24, 3), (512, 64, 4, 3), (2048, 512, 5, 1), (512, 512, 6, 2)):
        S, u = E.gl_case(n_fft, hop, T, B=B)
        Sd, ud = dev(S), dev(u)
        y = Au.griffin_lim(Sd, n_fft, hop, iters, ud)
        assert torch.equal(y, Au.griffin_lim(Sd, n_fft, hop, iters, ud)), (n_fft, hop, T)
        for b in range(B):
            assert torch.equal(y[b:b + 1], Au.griffin_lim(Sd[b:b + 1].contiguous(), n_fft, hop, iters, ud[b:b + 1].contiguous())), (n_fft, hop, T, b)
    for n_mels, n_fft in ((80, 1024), (40, 512)):
        mel = dev(E.m2l_input(n_mels, 11, 77, B=B))
        S = Au.mel_to_linear(mel, 22050, n_fft, n_mels)
        assert torch.equal(S, Au.mel_to_linear(mel, 22050, n_fft, n_mels))
        for b in range(B):
            assert torch.equal(S[b:b + 1], Au.mel_to_linear(mel[b:b + 1].contiguous(), 22050, n_fft, n_mels)), (n_mels, n_fft, b)
    rs = np.random.RandomState(21)
    for n_fft, hop, L in ((1024, 256, 256 * 19 + 37), (512, 200, 1777), (2048, 512, 1025)):
        y = dev(rs.randn(B, L).astype(np.float32))
        X = Au.stft(y, n_fft, hop)
        assert torch.equal(torch.view_as_real(X), torch.view_as_real(Au.stft(y, n_fft, hop)))
        for b in range(B):
            assert torch.equal(torch.view_as_real(X[b:b + 1]), torch.view_as_real(Au.stft(y[b:b + 1].contiguous(), n_fft, hop))), (n_fft, hop, L, b)
    for L, k in ((3 * 2048 + 5, 0.97), (2049, 0.999), (2047, -0.5)):
        x = dev(rs.randn(B, L).astype(np.float32))
        y = Au.inv_preemphasis(x, k)
        assert torch.equal(y, Au.inv_preemphasis(x, k))
        for b in range(B):
            assert torch.equal(y[b:b + 1], Au.inv_preemphasis(x[b:b + 1].contiguous(), k)), (L, k, b)


# ----------------------------------------------------------------------------------------------------------------------
# stft
# ----------------------------------------------------------------------------------------------------------------------
# measured max|X - X64| / max|X64| (bound 2e-5, the one of tests/test_gpu_audio.py):
# (kernels unmeasured on these cases; tests/test_gpu_audio.py's three cases pass the same bound)
@pytest.mark.parametrize("n_fft,hop,L,B", [
    (1024, 256, 256 * 19 + 100, 2), (512, 128, 128 * 30 + 1, 2), (2048, 512, 512 * 9 + 511, 2),      # L not a multiple of hop
    (512, 128, 257, 2), (1024, 256, 513, 2), (2048, 512, 1025, 2),                                    # the minimal L = n_fft/2 + 1
    (1024, 200, 5000, 2), (512, 200, 1777, 2), (2048, 300, 7001, 2), (1024, 1500, 6000, 2),           # hops that do not divide n_fft
    (1024, 256, 256 * 19, 7), (512, 64, 2000, 7)])                                                    # B = 7
def test_stft_envelope(n_fft, hop, L, B):
    rs = np.random.RandomState(n_fft + hop + L)
    y = rs.randn(B, L).astype(np.float32)
    X = Au.stft(dev(y), n_fft, hop).cpu().numpy()
    worst = 0.0
    for b in range(B):
        want = A.stft(y[b].astype(np.float64), n_fft, hop).T
        assert X[b].shape == want.shape == (1 + L // hop, n_fft // 2 + 1)
        worst = max(worst, float(np.abs(X[b] - want).max() / np.abs(want).max()))
    print(f"[stft {n_fft}/{hop} L={L} B={B}] max|X - X64| / max|X64| = {worst:.3e} (bound 2e-5)")
    assert worst <= 2e-5


# ----------------------------------------------------------------------------------------------------------------------
# mel_to_linear
# ----------------------------------------------------------------------------------------------------------------------
# measured: the worst position of the kernel's S inside its interval [lo, hi] (0 = the fp64 value, 1 = the interval's end), over
# T in {1, 11, 257} and both clips, and the number of entries that used the clamp rule:
# (kernels unmeasured; on the CPU: at most 0.002 % of a case's entries use the clamp rule, the median interval width is 3e-5 .. 6e-5 of S)
@pytest.mark.parametrize("T", [1, 11, 257])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
@pytest.mark.parametrize("n_mels", [40, 80])
def test_mel_to_linear_within_the_forward_error_bound(n_mels, n_fft, T):
    """S = max(inv @ amp, 1e-10)^1.5 must lie in the image of [acc64 - E, acc64 + E], E the forward-error bound of the fp32
    sum and of the fp32 amplitudes (E.m2l_bounds).  Inputs hold exact 0 and 1 and values outside [0, 1]; the entries excused
    by the clamp rule are capped at 1 %, none with acc64 > 1e-8."""
    mel = E.m2l_input(n_mels, T, E.m2l_seed(n_mels, n_fft, T))
    S = Au.mel_to_linear(dev(mel), 22050, n_fft, n_mels).cpu().numpy().astype(np.float64)      # (B, T, F)
    assert S.shape == (mel.shape[0], T, n_fft // 2 + 1) and np.isfinite(S).all()
    for b in range(mel.shape[0]):
        S64, lo, hi, straddles, acc = E.m2l_bounds(mel[b], 22050, n_fft, n_mels)
        got = S[b].T
        pos = np.where(got >= S64, (got - S64) / (hi - S64), (S64 - got) / (S64 - lo))
        print(f"[m2l {n_mels}/{n_fft} T={T} clip={b}] worst position in [lo, hi]: {pos.max():.3f}; clamp rule used by {int(straddles.sum())} of "
              f"{straddles.size}; clamped in fp64: {(acc <= E.CLAMP).mean():.2f}; median (hi - lo) / S = {np.median((hi - lo) / S64):.1e}")
        assert straddles.mean() <= E.M2L_CLAMP_CAP and not (straddles & (acc > 1e-8)).any()
        assert ((lo <= got) & (got <= hi)).all(), (b, float(pos.max()))


# ----------------------------------------------------------------------------------------------------------------------
# inverse pre-emphasis
# ----------------------------------------------------------------------------------------------------------------------
# bound = 4 x (the sequential numpy-fp32 recurrence's error against fp64) + 1e-9 max|y|.  The two numbers, worst case per k over
# the six lengths and four inputs, and the kernel's measured error beside them (all absolute, with max|y| of that case):
#   k = 0      fp32 recurrence 0 (the identity)      truncation 1e-9 max|y| = 4e-9
#   k = 0.97   fp32 recurrence <= 3.1e-5 (constant, max|y| 23.3)    truncation 2.3e-8
#   k = -0.5   fp32 recurrence <= 2.1e-7 (noise, max|y| 4.5)        truncation 4.5e-9
#   k = 0.999  fp32 recurrence <= 1.2e-2 (constant, max|y| 688)     truncation 6.9e-7 (none in fact: the warm-up covers the clip)
# (kernel errors unmeasured)
@pytest.mark.parametrize("k", E.PRE_KS)
@pytest.mark.parametrize("L", E.PRE_LENGTHS)
def test_inv_preemphasis_envelope(L, k):
    """Lengths around the kernel's 2048-sample chunks; k = 0 (identity), the reference's 0.97, a negative k, and 0.999 whose
    warm-up (20 700 samples) exceeds every length here; a constant, a slow sine, the impulse response and noise in one batch."""
    inputs = E.pre_inputs(L)
    x = np.stack(list(inputs.values()))
    got = Au.inv_preemphasis(dev(x), k).cpu().numpy()
    assert got.shape == x.shape and np.isfinite(got).all()
    fails = []
    for row, name in enumerate(inputs):
        y64, bound, e32 = E.pre_bound(x[row], k)
        err = float(np.abs(got[row] - y64).max())
        print(f"[pre L={L} k={k} {name}] err={err:.3e} bound={bound:.3e} (fp32 recurrence {e32:.3e}, truncation {1e-9 * np.abs(y64).max():.1e}) max|y|={np.abs(y64).max():.3e}")
        if not err <= bound:
            fails.append((name, err, bound))
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
# at 60 iterations on the harmonic clip (T = 64), oracle from fp64 magnitudes on the CPU: e0 = 0.6526, e60 = 0.18722184, spread under
# the perturbations 2e-9 (margin 1e-6); the numpy fp32 restatement reaches e60 = 0.18722183.  (kernels unmeasured)
def test_inv_mel_spectrogram_of_a_harmonic_signal():
    """The mel of a real harmonic signal (29 harmonics of a 110 -> 150 Hz glide), inverted at the reference's 60 iterations.
    The relative spectral error | |stft(y)| - S | / |S| of the kernels' waveform, measured in fp64, must not exceed that of the
    oracle run from the same magnitudes and phases by more than 512 x the spread of the oracle's own e60 under 2^-24
    perturbations of S (the multiple of the trajectory tests).  The wrapper is its parts: inv_mel_spectrogram is bit for bit
    inv_preemphasis(griffin_lim(mel_to_linear(mel))), and its waveform is the oracle's filter of that Griffin-Lim output."""
    mel = H.forward64(H.signals()["harmonic"])[0].astype(np.float32)                          # (80, 64)
    T = mel.shape[1]
    u = np.random.RandomState(3).rand(1, T, 513).astype(np.float32)
    Sd = Au.mel_to_linear(dev(mel[None]))
    S = Sd.cpu().numpy()[0].astype(np.float64)                                                # (T, F): what Griffin-Lim is given
    S64, lo, hi, straddles, acc = E.m2l_bounds(mel, 22050, 1024, 80)
    assert ((lo <= S.T) & (S.T <= hi)).all()

    def spec_err(y):
        return float(np.linalg.norm(np.abs(A.stft(np.asarray(y, np.float64), 1024, 256)).T - S) / np.linalg.norm(S))
    y0 = Au.griffin_lim(Sd, 1024, 256, 0, dev(u)).cpu().numpy()[0]
    y60 = Au.griffin_lim(Sd, 1024, 256, 60, dev(u))
    e0, e60 = spec_err(y0), spec_err(y60.cpu().numpy()[0])
    u64 = u[0].T.astype(np.float64)
    e60_oracle = spec_err(A.griffin_lim(S.T, 1024, 256, 60, u64))
    spread = 0.0
    for seed in range(E.GL_SEEDS):
        r = np.random.RandomState(1000 + seed).randn(*S.T.shape)
        spread = max(spread, abs(spec_err(A.griffin_lim(S.T * (1.0 + E.U32 * r), 1024, 256, 60, u64)) - e60_oracle))
    margin = E.GL_MULTIPLE * spread
    print(f"[e2e harmonic] e0={e0:.6f} e60 kernels={e60:.10f} e60 oracle={e60_oracle:.10f} difference={e60 - e60_oracle:+.3e} "
          f"oracle spread={spread:.3e} margin={margin:.3e}")
    assert e60 <= e60_oracle + margin, (e60, e60_oracle, margin)
    wav = Au.inv_mel_spectrogram(mel, 22050, 1024, 256, 80, angles0=u)
    assert wav.dtype == np.float32 and wav.shape == (256 * (T - 1),)
    assert np.array_equal(wav, Au.inv_preemphasis(y60).cpu().numpy()[0])
    y64, bound, e32 = E.pre_bound(y60.cpu().numpy()[0], A.PREEMPHASIS)
    err = float(np.abs(wav - y64).max())
    print(f"[e2e harmonic] waveform against the oracle's filter of the same Griffin-Lim output: err={err:.3e} bound={bound:.3e}")
    assert err <= bound
