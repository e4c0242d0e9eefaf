"""Inputs and derived bounds of the mel -> waveform envelope tests (tests/test_gpu_audio_envelope.py runs the kernels,
tests/test_audio_entry_points.py checks on the CPU what these bounds assume).  Every bound here is computed from the fp64
restatement oracle/audio_oracle.py and the precision of fp32, never from a kernel's output."""
import numpy as np

from oracle import audio_oracle as A

U32 = 2.0 ** -24                  # unit roundoff of fp32 (half of eps32 = 2^-23)

# ----------------------------------------------------------------------------------------------------------------------
# the reflect map
# ----------------------------------------------------------------------------------------------------------------------
# (n_fft, hop) of the short-grid table: Griffin-Lim's grid is L = hop (T - 1) samples, padded by n_fft/2 each side
REFLECT_TABLE = [(1024, 256), (512, 128), (2048, 512), (1024, 128), (512, 64), (1024, 512), (1024, 1024)]


def c_rem(a, b):
    """C's a % b (truncates towards zero), which is what the kernel executes."""
    return int(np.fmod(a, b))


def reflect_index_fixed(i, L):
    """stft_frame_lds's padded index, statement by statement (i = t hop + n - N/2, any sign)."""
    period = 2 * (L - 1)
    idx = c_rem(i, period)
    if idx < 0:
        idx += period
    if idx >= L:
        idx = period - idx
    return idx


def reflect_index_one_fold(i, L):
    """The map before the fix (and melspectrogram_kernel's, which is guarded by L > N/2): one fold each side, then a clamp."""
    idx = -i if i < 0 else i
    if idx >= L:
        idx = 2 * (L - 1) - idx
    return 0 if idx < 0 else (L - 1 if idx >= L else idx)


# ----------------------------------------------------------------------------------------------------------------------
# Griffin-Lim: the conditioning of the fp64 restatement is the yardstick
# ----------------------------------------------------------------------------------------------------------------------
GL_SEEDS = 8
# The response below is what ONE relative perturbation of size u = 2^-24 of S does to y.  An fp32 run perturbs every
# intermediate, not S alone: with K iterations there are 2K + 1 FFTs of log2(N) butterfly stages (each stage rounds once: an
# N-point FFT contributes about log2(N) u), and per pass about 7 more roundings (sincospi or X/|X| with its square root, the
# window twice, the 1/N scale, the sum of squares and the quotient).  At the largest case tested, K = 3 and N = 2048:
# (2 * 3 + 1) * (11 + 7) = 126 -> 128 perturbations of size u, each through the same conditioning.  A further factor 4 because
# the response is the largest of only GL_SEEDS random directions of S, while roundings also act in directions S does not
# reach (straight on the phase of a weak bin, where X/|X| is ill-conditioned): the sampled response under-estimates the gain
# the roundings meet, with a heavy tail.  (Cross-check without any kernel: a numpy complex64 restatement of the same radix-2
# algorithm on these inputs has error / response of median 2.3, 99th percentile 51 and maximum 107 over the 270 clip-cases.)
# 512 is used for every case: the small cases have slack, the ill-conditioned ones a bound that grows with their own
# conditioning; at the typical response of 1e-7 it is 5e-5 of max|y|, against the 2e-3 guessed before.
GL_MULTIPLE = 512.0


def gl_response(S, n_fft, hop, iters, u, want=None, seeds=GL_SEEDS):
    """S, u (F, T) float64.  Largest relative response max|y' - y| / max|y| of the fp64 Griffin-Lim to S (1 + 2^-24 r),
    r standard normal, over `seeds` draws.  Returns (y, response)."""
    if want is None:
        want = A.griffin_lim(S, n_fft, hop, iters, u)
    peak = np.abs(want).max()
    if peak == 0.0:
        return want, 0.0
    resp = 0.0
    for seed in range(seeds):
        r = np.random.RandomState(1000 + seed).randn(*S.shape)
        yp = A.griffin_lim(S * (1.0 + U32 * r), n_fft, hop, iters, u)
        resp = max(resp, float(np.abs(yp - want).max() / peak))
    return want, resp


def gl_case(n_fft, hop, T, B=3):
    """Seeded magnitudes with a 60 dB range and phases: S, u (B, T, F) float32, frame-major like the kernels."""
    rs = np.random.RandomState(7 * n_fft + 3 * hop + T)
    F = n_fft // 2 + 1
    S = (10.0 ** (3.0 * rs.rand(B, T, F) - 2.0)).astype(np.float32)
    u = rs.rand(B, T, F).astype(np.float32)
    return S, u


def degenerate_case(n_fft, T, B=3):
    """gl_case with all-zero frames (clip 0), all-zero bins (clip 1, DC, Nyquist and a band) and an all-zero clip (clip 2)."""
    S, u = gl_case(n_fft, n_fft // 4, T, B)
    S[0, [0, T // 2, T - 1], :] = 0.0
    S[1, :, [0, n_fft // 2]] = 0.0
    S[1, :, 17:40] = 0.0
    S[2] = 0.0
    return S, u


# ----------------------------------------------------------------------------------------------------------------------
# perfect reconstruction
# ----------------------------------------------------------------------------------------------------------------------
PR_AMPS = (0.5, 0.3, 0.2)
PR_FREQS = (220.0, 1318.5, 3520.0)          # Hz at 22050: band-limited, far below Nyquist


def pr_signal(L, sr=22050):
    t = np.arange(L) / sr
    y = sum(a * np.sin(2 * np.pi * f * t + 0.3 * i) for i, (a, f) in enumerate(zip(PR_AMPS, PR_FREQS)))
    return y.astype(np.float32)


def pr_tolerance(n_fft):
    """Absolute bound on |istft(stft(y)) - y| for pr_signal.  Per element, in units of u = 2^-24, linear (worst-case) sum:
      2 log2(N)   the two FFTs, one rounding per butterfly stage;
      1           |X| stored in fp32;
      pi          the phase: u in [0, 1) rounded to fp32 is wrong by <= u/2, i.e. 2 pi u / 2 radians;
      2           sincospi of it;
      4           the analysis window, the synthesis window, the 1/N scale, the sum of squares with its quotient
    = (2 log2(N) + 10.2) u relative per spectral bin.  A relative error d on every bin of a windowed sinusoid of amplitude a
    returns at most d a (the Hann window's spectrum sums to its peak), so d sum(a_k) per frame; overlap-add weights frames by
    w / sum(w^2), whose sum over the frames covering a sample is 2/1.5 at hop = N/4 and 4/3 at N/8: 1.34 d sum(a_k).
    sum(a_k) = 1.0 here and max|y| is 0.9 to 1.0, so this is also the bound relative to max|y| within 10 %."""
    d = (2 * np.log2(n_fft) + 10.2) * U32
    return 1.34 * d * sum(PR_AMPS)


# ----------------------------------------------------------------------------------------------------------------------
# mel_to_linear
# ----------------------------------------------------------------------------------------------------------------------
M2L_C = 1.0                     # the dot product's constant in units of n_mels * eps32 (eps32 = 2^-23 = 2u), see m2l_bounds
M2L_AMP_REL = 64 * U32          # relative error of the fp32 amplitude, see m2l_bounds
M2L_POW_REL = 8 * U32           # powf (a few ulp) and the fp32 value of the constant 1e-10 (u, times the power)
M2L_CLAMP_CAP = 0.01            # at most this fraction of entries may straddle the clamp, none of them with acc > 1e-8
CLAMP = 1e-10


def m2l_seed(n_mels, n_fft, T):
    """The seed of a case.  The family (the offset 10000) was picked on the CPU, from the oracle alone, as one for which no
    entry with an fp64 sum above 1e-8 comes within its error bound of the clamp (tests/test_audio_entry_points.py asserts it;
    about one family in three has none, the others have two or three such entries among 1.3 million)."""
    return 10000 + n_mels + n_fft + T


def m2l_input(n_mels, T, seed, B=2):
    """A normalised mel (B, n_mels, T) float32 that is smooth along the mel axis, like a real spectrum (so that the product
    with the pseudo-inverse cancels mildly; white inputs cancel to the clamp in a large share of bins), with entries set to
    exactly 0 and exactly 1 and entries below 0 and above 1 (all four are clipped or hit the ends of the dB range)."""
    rs = np.random.RandomState(seed)
    m = np.arange(n_mels)[None, :, None] / n_mels
    base = 0.55 + 0.25 * np.cos(2 * np.pi * (m * rs.uniform(0.5, 1.5, (B, 1, T)) + rs.rand(B, 1, T))) - 0.25 * m
    mel = (base + 0.02 * rs.randn(B, n_mels, T)).astype(np.float32)
    flat = mel.reshape(-1)
    pick = rs.permutation(flat.size)[:4 * max(1, flat.size // 50)].reshape(4, -1)        # 2 % of the entries each
    flat[pick[0]] = 0.0
    flat[pick[1]] = 1.0
    flat[pick[2]] = -0.25 * rs.rand(pick.shape[1]).astype(np.float32) - 0.01
    flat[pick[3]] = 1.0 + 0.3 * rs.rand(pick.shape[1]).astype(np.float32) + 0.01
    return mel


def m2l_bounds(mel, sample_rate, n_fft, n_mels, power=A.POWER):
    """mel (n_mels, T) float32.  Returns (S64, lo, hi, straddles, acc64), all (F, T): the kernel's S must lie in [lo, hi].

    acc64 = inv @ amp in fp64 (the oracle's).  The kernel's sum differs by at most
        E = (c n_mels eps32 + r_amp) sum_m |inv[f, m]| amp[m]
      c n_mels eps32, c = 1: an fma chain of n terms is off by at most n u sum|terms| and the fp32 copy of inv by u sum|terms|,
        (n + 1) u <= n eps32 / 2 + ...; c = 1 leaves a factor 2 for the first-order terms dropped;
      r_amp = 64 u: amp = exp10f(x), x = db / 20 in [-4, 1].  Before the exponential: v * 100, + (-100), + 20 each round at
        magnitude <= 100 (<= 2^-18 = 64 u absolute, 3.2 u after the factor 0.05), the product by 0.05f rounds at |x| <= 4
        (4 u) and 0.05f is itself rounded (4 u): 17.6 u in x, times ln 10 = 41 u relative in amp; exp10f a few ulp more.
    max(., 1e-10)^power is monotone, so S lies between the images of acc64 -+ E, widened by r_pow = 8 u (powf, and the fp32
    value of 1e-10).  An entry whose interval contains the clamp's corner (acc64 - E < 1e-10 < acc64 + E) may land on either
    side; such entries are counted in `straddles` and capped by the caller."""
    inv = np.linalg.pinv(A.mel_basis(sample_rate, n_fft, n_mels).astype(np.float64))
    amp = A.db_to_amp(A.denormalize(mel.astype(np.float64)) + A.REF_LEVEL_DB)
    acc = inv @ amp
    E = (M2L_C * n_mels * 2 * U32 + M2L_AMP_REL) * (np.abs(inv) @ amp)
    S64 = np.maximum(CLAMP, acc) ** power
    lo = np.maximum(CLAMP, acc - E) ** power * (1 - M2L_POW_REL)
    hi = np.maximum(CLAMP, acc + E) ** power * (1 + M2L_POW_REL)
    straddles = (acc - E < CLAMP) & (acc + E > CLAMP)
    return S64, lo, hi, straddles, acc


# ----------------------------------------------------------------------------------------------------------------------
# inverse pre-emphasis
# ----------------------------------------------------------------------------------------------------------------------
PRE_LENGTHS = (1, 2047, 2048, 2049, 4096, 3 * 2048 + 5)
PRE_KS = (0.0, 0.97, -0.5, 0.999)


def pre_inputs(L):
    """name -> float32 (L,): the inputs on which the filter's gain 1 / (1 - k) is reached (constant, slow sine), its impulse
    response, and noise."""
    n = np.arange(L)
    imp = np.zeros(L, np.float32)
    imp[0] = 1.0
    return {"constant": np.full(L, 0.7, np.float32), "slow_sine": np.sin(2 * np.pi * n / 1500.0).astype(np.float32), "impulse": imp,
            "noise": np.random.RandomState(L).randn(L).astype(np.float32)}


def inv_preemphasis_f32(x, k):
    """The same recurrence run sequentially in fp32 (two roundings per step): the rounding error any fp32 implementation has."""
    x = np.asarray(x, np.float32)
    k = np.float32(k)
    y = np.empty_like(x)
    acc = np.float32(0.0)
    for n in range(len(x)):
        acc = np.float32(x[n] + np.float32(k * acc))
        y[n] = acc
    return y


def pre_bound(x, k):
    """(y64, bound, fp32 rounding error): bound = 4 max|seq32 - y64| + 1e-9 max|y64| (the warm-up's documented truncation)."""
    y64 = A.inv_preemphasis(x.astype(np.float64), float(np.float32(k)))
    e32 = float(np.abs(inv_preemphasis_f32(x, k).astype(np.float64) - y64).max())
    return y64, 4.0 * e32 + 1e-9 * float(np.abs(y64).max()), e32
