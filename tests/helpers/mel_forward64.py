"""fp64 statement of the wav -> mel front end (src/audio_tacotron.py:70-78 with hparams_tacotron.py's settings), composed
from what oracle/audio_oracle.py already restates (stft, mel_basis, the constants) plus the four remaining lines in numpy
float64; the seeded test signals; and the derived amplitude-domain bound the kernel is held to.  parity unpinned, as for the
export: librosa is absent, so the reference's own function cannot be run."""
import numpy as np

from oracle import audio_oracle as A

SR = 22050
L_DEFAULT = 256 * 63
REL = 2e-5            # the STFT bound of tests/test_gpu_audio.py::test_stft_matches_numpy, relative to the spectrum's peak
OUT_LO_AMP, OUT_HI_AMP = 1e-4, 10.0     # the amplitudes at which the normalised value clips to 0 and to 1 (see amplitude_of)


def rescale(y):
    y = np.asarray(y, dtype=np.float32)
    return (y / np.abs(y).max() * 0.999).astype(np.float32)


def signals(L=L_DEFAULT):
    """name -> float32 clip of L samples (each rescaled to a peak of 0.999 except 'faint')."""
    t = np.arange(L) / SR
    noise = 0.3 * np.random.RandomState(0).randn(L)
    rs = np.random.RandomState(1)
    f0 = 110.0 + 40.0 * t / max(t[-1], 1e-9)                                   # chirp 110 -> 150 Hz
    phase = 2 * np.pi * np.cumsum(f0) / SR
    harm = sum(np.sin(h * phase) / h for h in range(1, 30))                    # 29 harmonics
    harm = harm * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 1e-3 * rs.randn(L)
    sine = np.sin(2 * np.pi * 440.0 * t)
    half = 0.3 * np.random.RandomState(2).randn(L)
    half[L // 2:] = 0.0
    faint = (1e-4 * np.random.RandomState(3).randn(L)).astype(np.float32)
    return {"noise": rescale(noise), "harmonic": rescale(harm), "sine": rescale(sine), "half_zero": rescale(half), "faint": faint}


def forward64(y, n_fft=1024, hop=256, n_mels=80, sample_rate=SR):
    """y: the float32 samples the kernel gets.  Returns (out (n_mels, T) normalised, m (n_mels, T) mel amplitudes,
    max |X|, row sums of the basis (n_mels,)), all float64."""
    y = np.asarray(y, dtype=np.float64)
    p = y.copy()
    p[1:] -= A.PREEMPHASIS * y[:-1]                                            # lfilter([1, -k], [1], y)
    X = np.abs(A.stft(p, n_fft, hop))                                          # (F, T)
    basis = A.mel_basis(sample_rate, n_fft, n_mels).astype(np.float64)
    m = basis @ X
    S = 20 * np.log10(np.maximum(10.0 ** (A.MIN_LEVEL_DB / 20), m)) - A.REF_LEVEL_DB
    out = np.clip(A.MAX_ABS_VALUE * (S - A.MIN_LEVEL_DB) / (-A.MIN_LEVEL_DB), 0, A.MAX_ABS_VALUE)
    return out, m, float(X.max()), basis.sum(axis=1)


def amplitude_of(out):
    """Undo the normalisation: out = (20 log10 m - 20 + 100) / 100  =>  m = 10^((100 out - 80) / 20).  out = 0 is m = 1e-4 and
    out = 1 is m = 10: what an output can show of m is clip(m, 1e-4, 10)."""
    return 10.0 ** ((100.0 * np.asarray(out, dtype=np.float64) - 80.0) / 20.0)


def check_amplitude(out_gpu, y, n_fft=1024, hop=256, n_mels=80, tag=""):
    """Every entry, derived tolerance: |m_gpu - m_ref| <= delta_b + 2e-5 m_ref with delta_b = 2e-5 max|X_ref| sum_f basis[b, f]
    (2e-5 of the spectrum's peak pushed through a non-negative linear map, plus 2e-5 relative for the dB arithmetic and this
    inversion).  An output shows m only through clip(m, 1e-4, 10), which is 1-Lipschitz, so both sides are compared clipped:
    where the reference clips to 0 this reads m_gpu <= 1e-4 + delta_b (+ 2e-9), where it clips to 1, m_gpu >= 10 - delta_b
    (asserted in that stricter form).  Returns (out_ref, m_ref, delta, worst |m_gpu - m_ref| / bound)."""
    out_ref, m_ref, xmax, rows = forward64(y, n_fft, hop, n_mels)
    assert out_gpu.shape == out_ref.shape, (tag, out_gpu.shape, out_ref.shape)
    delta = (REL * xmax * rows)[:, None]
    m_gpu = amplitude_of(out_gpu)
    m_clip = np.clip(m_ref, OUT_LO_AMP, OUT_HI_AMP)
    bound = delta + REL * m_clip
    err = np.abs(m_gpu - m_clip)
    worst = float((err / bound).max())
    print(f"[{tag}] amplitude check: worst |m_gpu - m_ref| / bound = {worst:.3e}; max |d out| = {np.abs(out_gpu - out_ref).max():.3e}; "
          f"entries clipped to 0: {(out_ref == 0).sum()}, to 1: {(out_ref == 1).sum()} of {out_ref.size}")
    assert (err <= bound).all(), (tag, worst)
    hi = m_ref >= OUT_HI_AMP
    assert (m_gpu[hi] >= (OUT_HI_AMP - np.broadcast_to(delta, m_ref.shape)[hi])).all(), tag
    return out_ref, m_ref, delta, worst
