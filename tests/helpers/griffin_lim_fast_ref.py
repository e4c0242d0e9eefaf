"""The fp64 restatement of include/nsg.h's nsg_audio_griffin_lim_fast and nsg_audio_spectral_convergence, on the oracle's own
stft / istft (imported from oracle/audio_oracle.py, neither copied nor edited), with the inputs and the derived bounds that
tests/test_griffin_lim_fast_host.py (CPU) and tests/test_gpu_griffin_lim_fast.py share.  Every bound here comes from the fp64
restatement and the precision of fp32, never from a kernel's output."""
import numpy as np
import torch

from oracle.audio_oracle import istft, stft
from tests.helpers import audio_envelope as E

U32 = E.U32


def unit_phase(t):
    """t / |t| with np.angle(0) = 0: exp(i angle(t)) without the trigonometric round trip."""
    mag = np.abs(t)
    return np.where(mag > 0, t / np.where(mag > 0, mag, 1.0), 1.0 + 0.0j)


def griffin_lim_fast(S, n_fft, hop, iters, u, momentum, want_state=False):
    """S, u (F, T) float64, the oracle's orientation.  X_0 = 0, y_0 = istft(S exp(2 pi i u)); for i = 1 .. iters:
    X_i = stft(y_{i-1}), t_i = X_i + momentum (X_i - X_{i-1}), y_i = istft(S t_i / |t_i|).  Returns y_iters [, X_iters (None at 0)]."""
    Sc = np.abs(S).astype(np.complex128)
    y = istft(Sc * np.exp(2j * np.pi * u), hop)
    prev, X = np.zeros(S.shape, dtype=np.complex128), None
    for _ in range(iters):
        X = stft(y, n_fft, hop)
        t = X + momentum * (X - prev)
        prev = X
        y = istft(Sc * unit_phase(t), hop)
    return (y, X) if want_state else y


def convergence_sums(y, S, n_fft, hop):
    """y (hop (T - 1),), S (F, T) float64 -> (T, 2): per frame { sum_f (|X| - S)^2, sum_f S^2 }, X = stft(y)."""
    X = stft(y, n_fft, hop)
    assert X.shape == S.shape, (X.shape, S.shape)
    return np.stack((((np.abs(X) - S) ** 2).sum(0), (S ** 2).sum(0)), axis=1)


def figure(sums):
    """sqrt(num / den) of a (..., 2) array of sums; 0 where both are 0, inf where only den is 0."""
    num, den = np.asarray(sums)[..., 0], np.asarray(sums)[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num == 0, 0.0, np.sqrt(num / den))


def spectral_convergence(y, S, n_fft, hop):
    return float(figure(convergence_sums(y, S, n_fft, hop).sum(0)))


def gl_fast_response(S, n_fft, hop, iters, u, momentum, seeds=E.GL_SEEDS):
    """audio_envelope.gl_response with this restatement at `momentum`: (y, X_iters, the largest relative response of y to
    S (1 + 2^-24 r) over `seeds` draws, the same for X_iters relative to max|X_iters|)."""
    want, X = griffin_lim_fast(S, n_fft, hop, iters, u, momentum, want_state=True)
    peak = np.abs(want).max()
    if peak == 0.0:
        return want, X, 0.0, 0.0
    resp, resp_x = 0.0, 0.0
    for seed in range(seeds):
        r = np.random.RandomState(1000 + seed).randn(*S.shape)
        yp, Xp = griffin_lim_fast(S * (1.0 + U32 * r), n_fft, hop, iters, u, momentum, want_state=True)
        resp = max(resp, float(np.abs(yp - want).max() / peak))
        if X is not None:
            resp_x = max(resp_x, float(np.abs(Xp - X).max() / np.abs(X).max()))
    return want, X, resp, resp_x


# ----------------------------------------------------------------------------------------------------------------------
# the convergence claim's signal
# ----------------------------------------------------------------------------------------------------------------------
HARM_SR, HARM_NFFT, HARM_HOP, HARM_T = 22050, 512, 128, 64


def harmonic_case():
    """(y, S (F, T), u (F, T)) float64: a gliding harmonic tone with tremolo and a little noise, L = 128 * 63 samples at 22 050 Hz;
    f0(t) = 120 + 60 sin(2 pi 1.5 t), the phase the running sum of 2 pi f0 / sr, harmonics 1 .. 11 at amplitude 1 / k, times
    0.5 + 0.5 sin^2(2 pi 3 t), plus 0.01 RandomState(0).randn; S = |stft(y)|, u = RandomState(1).rand."""
    L = HARM_HOP * (HARM_T - 1)
    t = np.arange(L) / HARM_SR
    phase = np.cumsum(2 * np.pi * (120.0 + 60.0 * np.sin(2 * np.pi * 1.5 * t)) / HARM_SR)
    y = sum(np.sin(k * phase) / k for k in range(1, 12)) * (0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * t) ** 2)
    y = y + 0.01 * np.random.RandomState(0).randn(L)
    S = np.abs(stft(y, HARM_NFFT, HARM_HOP))
    u = np.random.RandomState(1).rand(*S.shape)
    return y, S, u


# ----------------------------------------------------------------------------------------------------------------------
# the spectral-convergence bound
# ----------------------------------------------------------------------------------------------------------------------
def sc_eps(n_fft):
    """eps of |sc_dev - sc_64| <= eps (1 + sc_64).

    sc = sqrt(num) / ||S||, sqrt(num) = || |X| - S || over the clip's bins.  The device differs from fp64 in |X| alone (S is the
    same fp32 array on both sides, and the fp64 sums of at most 2^20 terms are off by 2^-53 a term): d|X| per bin.
      * An N-point radix-2 fp32 FFT rounds once per butterfly stage; its error is about log2(N) u in norm, u = 2^-24
        (audio_envelope.pr_tolerance counts it the same way).  Taken twice, 2 log2(N) u, for the window product in front of it
        (sin^2 of a rounded argument, and the product) and the first-order terms dropped.
      * |X| = sqrtf(re^2 + im^2): two products, a sum and a root, each u relative or less: 4 u.  fl32(|X| - S): u of a
        difference that is at most |X| + S; counted as 2 u of |X| and 2 u of S.
    So || d|X| || <= (2 log2 N + 6) u ||X|| + 2 u ||S||, and ||X|| <= ||S|| + sqrt(num) (the triangle inequality on |X| = S +
    (|X| - S)): || d|X| || <= (2 log2 N + 8) u (||S|| + sqrt(num)) = eps (||S|| + sqrt(num)).  sqrt(num) is a norm, so it moves by at
    most || d|X| ||; divided by ||S||: |sc_dev - sc_64| <= eps (1 + sc_64)."""
    return (2 * np.log2(n_fft) + 8) * U32


def frames32(y, n_fft, hop):
    """The windowed, reflect-padded frames of y in fp32: (T, n_fft) float32 with the oracle's framing."""
    yp = np.pad(np.asarray(y, np.float32), n_fft // 2, mode="reflect")
    T = 1 + (len(yp) - n_fft) // hop
    n = np.arange(n_fft, dtype=np.float32)
    w = np.sin(np.float32(np.pi) * n / np.float32(n_fft)).astype(np.float32) ** 2
    return np.stack([yp[t * hop:t * hop + n_fft] * w for t in range(T)]).astype(np.float32)


def convergence_sums_c64(y, S, n_fft, hop):
    """convergence_sums restated in fp32: float32 frames, a complex64 FFT (torch.fft.rfft on the CPU), |X| and the difference in
    fp32, the squares and sums in fp64.  No kernel is involved: this shows what an fp32 implementation reaches."""
    X = torch.fft.rfft(torch.from_numpy(frames32(y, n_fft, hop)), dim=1)
    assert X.dtype == torch.complex64
    X = X.numpy().T
    mag = np.sqrt(X.real * X.real + X.imag * X.imag).astype(np.float32)
    S32 = np.asarray(S, np.float32)
    e = (mag - S32).astype(np.float32).astype(np.float64)
    return np.stack(((e * e).sum(0), (S32.astype(np.float64) ** 2).sum(0)), axis=1)


def band_limited_case(n_fft, hop, T):
    """(y float32, S float32 (F, T)): audio_envelope.pr_signal on Griffin-Lim's grid and S = |stft64(y)| rounded to fp32, for which
    the true figure is the rounding of S alone, below 2^-24, and the device's at most sc_eps."""
    y = E.pr_signal(hop * (T - 1))
    S = np.abs(stft(y.astype(np.float64), n_fft, hop)).astype(np.float32)
    return y, S


# (n_fft, hop, T) of the GPU test's gl_case inputs, the issue's list
GL_FAST_CASES = [(512, 128, 2), (512, 128, 5), (512, 64, 9), (1024, 256, 24), (2048, 512, 9), (1024, 1024, 4)]
GL_FAST_ITERS = (1, 3)
GL_FAST_MOMENTA = (0.5, 0.99)
