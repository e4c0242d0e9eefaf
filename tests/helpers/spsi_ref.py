"""The numpy fp64 restatement of include/nsg.h's nsg_audio_spsi_phases (single-pass spectrogram inversion phases), operation for
operation in the header's order, with the inputs that tests/test_spsi_host.py (CPU) and tests/test_gpu_spsi.py share.  Nothing
here comes from a kernel's output."""
import numpy as np

from oracle.audio_oracle import istft, stft

NFFTS = (512, 1024, 2048)


def frac(x):
    return x - np.floor(x)


def peaks_of(m):
    """The peaks of one frame of fp32 magnitudes: bins j in 1 .. F-2 with m[j] > m[j-1] and m[j] > m[j+1], strict."""
    m = np.asarray(m, np.float32)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((m[1:-1] > m[:-2]) & (m[1:-1] > m[2:])) + 1


def peak_offsets(m, peaks):
    a, b, c = (np.asarray(m, np.float32)[peaks + d].astype(np.float64) for d in (-1, 0, 1))
    with np.errstate(all="ignore"):
        return 0.5 * (a - c) / ((a - 2.0 * b) + c)


def owners(m, peaks):
    """(F,) the peak that owns each bin: between consecutive peaks j < j' the bins up to the FIRST minimum of m[j .. j'] are j's."""
    m = np.asarray(m, np.float32)
    own = np.empty(len(m), dtype=np.int64)
    start = 0
    for i, j in enumerate(peaks):
        end = len(m) - 1 if i == len(peaks) - 1 else j + int(np.argmin(m[j:peaks[i + 1] + 1]))
        own[start:end + 1] = j
        start = end + 1
    return own


def spsi_phases(S, n_fft, hop, want_state=False):
    """S (T, F) fp32 magnitudes of one clip -> angles (T, F) float32 in turns in [0, 1) [, the states phi (T, F) float64]."""
    S = np.asarray(S, np.float32)
    T, F = S.shape
    assert F == n_fft // 2 + 1 and n_fft % hop == 0
    r = hop / n_fft                                   # a power of two: exact
    k = np.arange(F, dtype=np.float64)
    phi = np.zeros(F)
    out = np.empty((T, F), dtype=np.float32)
    states = np.empty((T, F))
    for t in range(T):
        m = S[t]
        pk = peaks_of(m)
        if len(pk) == 0:
            phi = frac(phi + k * r)
        else:
            val = phi[pk] + (pk.astype(np.float64) + peak_offsets(m, pk)) * r
            by_peak = np.empty(F)
            by_peak[pk] = val
            with np.errstate(invalid="ignore"):
                phi = frac(by_peak[owners(m, pk)])
        states[t] = phi
        with np.errstate(invalid="ignore"):
            f = frac(phi + 0.5 * k).astype(np.float32)
        f[f == np.float32(1.0)] = np.float32(0.0)
        out[t] = f
    return (out, states) if want_state else out


def spsi_batch(S, n_fft, hop):
    """S (B, T, F) -> (B, T, F) float32, clip by clip."""
    return np.stack([spsi_phases(s, n_fft, hop) for s in S])


# ----------------------------------------------------------------------------------------------------------------------
# Griffin-Lim from given phases and the figure it is judged by, on the oracle's stft / istft (fp64, (F, T) orientation)
# ----------------------------------------------------------------------------------------------------------------------
def griffin_lim(S, n_fft, hop, iters, u):
    """S, u (F, T) float64: y_0 = istft(S exp(2 pi i u)), then iters times y <- istft(S X / |X|), X = stft(y)."""
    y = istft(S * np.exp(2j * np.pi * u), hop)
    for _ in range(iters):
        X = stft(y, n_fft, hop)
        mag = np.abs(X)
        y = istft(S * np.where(mag > 0, X / np.where(mag > 0, mag, 1.0), 1.0), hop)
    return y


def spectral_convergence(y, S, n_fft, hop):
    return float(np.linalg.norm(np.abs(stft(y, n_fft, hop)) - S) / np.linalg.norm(S))


def harmonic_signal(n_fft, hop, T, harmonics, sr=22050, seed=0):
    """A gliding harmonic tone with amplitude modulation and a little noise, hop (T - 1) samples: f0(t) = 140 + 40 sin(2 pi 0.7 t),
    the phase the running sum of 2 pi f0 / sr, harmonics 1 .. `harmonics` at amplitude 1 / sqrt(h), times 0.6 + 0.4 sin(2 pi 2 t),
    plus 0.003 RandomState(seed).randn."""
    L = hop * (T - 1)
    t = np.arange(L) / sr
    phase = np.cumsum(2 * np.pi * (140.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)) / sr)
    y = sum(np.sin(h * phase) / np.sqrt(h) for h in range(1, harmonics + 1)) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.0 * t))
    return 0.1 * y + 0.003 * np.random.RandomState(seed).randn(L)


# the issue's trial: n_fft 1024, hop 256, 120 frames, 29 harmonics;  the GPU test's: n_fft 512, hop 128, 60 frames, 14 harmonics
TRIAL = dict(n_fft=1024, hop=256, T=120, harmonics=29)
POINT = dict(n_fft=512, hop=128, T=60, harmonics=14)


def trial_case(n_fft, hop, T, harmonics):
    """(S (F, T) float64 = the fp32-rounded true magnitudes of harmonic_signal, u (F, T) = RandomState(1).rand)."""
    S = np.abs(stft(harmonic_signal(n_fft, hop, T, harmonics), n_fft, hop)).astype(np.float32).astype(np.float64)
    return S, np.random.RandomState(1).rand(*S.shape)


def convergence_from(S, n_fft, hop, u, iters):
    return spectral_convergence(griffin_lim(S, n_fft, hop, iters, u), S, n_fft, hop)


# ----------------------------------------------------------------------------------------------------------------------
# the GPU test's magnitude patterns
# ----------------------------------------------------------------------------------------------------------------------
def patterns(n_fft, T, B, seed=0):
    """name -> (B, T, F) float32 magnitudes.  Every pattern is finite."""
    F = n_fft // 2 + 1
    rs = np.random.RandomState(seed + n_fft + 7 * T + B)
    k = np.arange(F)
    out = {}
    out["random"] = rs.rand(B, T, F).astype(np.float32) + np.float32(1e-3)
    two = np.full((B, T, F), 1.0, dtype=np.float32)                       # peaks at bins 1 and F-2 only, the valley one long plateau:
    two[:, :, 1] = two[:, :, F - 2] = 3.0                                 # m[1 .. F-2] = 3 1 1 ... 1 3, whose first minimum is bin 2
    two[:, :, 0] = two[:, :, F - 1] = 2.0
    out["two_peaks_plateau"] = two
    vee = (np.abs(k - (F // 2 + 3)) + 1.0).astype(np.float32)            # peaks at 1 and F-2 again, one strict valley off centre
    vee[0] = vee[1] - 1.0
    vee[F - 1] = vee[F - 2] - 1.0
    out["two_peaks_valley"] = np.broadcast_to(vee * (1.0 + rs.rand(B, T, 1)).astype(np.float32), (B, T, F)).copy()
    one = np.zeros((B, T, F), dtype=np.float32)
    for b in range(B):
        for t in range(T):
            j = 1 + (37 * b + 11 * t) % (F - 2)
            one[b, t, j] = 2.0 + rs.rand()
            one[b, t, j - 1] = rs.rand()
    out["one_peak"] = one
    out["zeros"] = np.zeros((B, T, F), dtype=np.float32)
    out["constant"] = np.full((B, T, F), 0.75, dtype=np.float32)
    out["ramp"] = np.broadcast_to((k + 1).astype(np.float32), (B, T, F)).copy()
    ties = np.tile(np.array([5, 3, 4, 4, 3, 5, 5, 2, 2, 6, 1, 6, 1, 1, 7, 0], dtype=np.float32), F // 16 + 1)[:F]
    out["plateaus_and_ties"] = np.broadcast_to(ties, (B, T, F)).copy()   # plateaus 4 4 / 5 5, valleys tied at 3 .. 3, 2 2, 1 .. 1 1
    scales = rs.rand(B, T, F).astype(np.float32) + np.float32(0.05)
    for t in range(T):
        scales[:, t] *= np.float32((1.0, 1e-42, 1.0, 1e30)[t % 4])       # a frame of denormals and a frame of 1e30 beside ordinary ones
    out["denormal_and_huge"] = scales
    alt = rs.rand(B, T, F).astype(np.float32) + np.float32(0.1)
    alt[:, 1::2] = np.linspace(2.0, 1.0, F, dtype=np.float32)            # every other frame a monotone ramp: no peak
    out["alternating"] = alt
    mov = np.full((B, T, F), 0.01, dtype=np.float32)
    for b in range(B):
        for t in range(T):
            j = 1 + (5 + 3 * b + t) % (F - 2)
            mov[b, t, j] = 1.0
            mov[b, t, j - 1] = 0.4 + 0.1 * b
            mov[b, t, j + 1] = 0.3
    out["moving_peak"] = mov
    return out
