"""fp64 statements of the resampler's and the silence trimmer's formulas (include/nsg.h: nsg_audio_resample,
nsg_audio_trim_bounds), written straight from the definitions: the resampler's sum is evaluated from h itself, with no
polyphase table, and I0 comes from scipy.special (the package uses numpy's).  parity unpinned: librosa and resampy are
absent, so these are what the kernels are held to; tests/test_resample_host.py checks this resampler against
scipy.signal.resample_poly with the same prototype filter."""
from math import gcd

import numpy as np
from scipy.special import i0

Z, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492


def ratio(sr_in, sr_out):
    g = gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g                        # P, Q


def half_width(P, Q):
    return Z if P >= Q else -(-Z * Q // P)                # W = ceil(Z / s), s = min(1, P / Q)


def h(u):
    """h(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u/Z)^2)) / I0(beta) for |u| < Z, else 0."""
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < Z
    r = np.where(inside, u / Z, 0.0)
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * u) * i0(BETA * np.sqrt(1.0 - r * r)) / i0(BETA), 0.0)


def resample64(x, sr_in, sr_out):
    """y[m] = sum_n x[n] s h(s (m Q - n P) / P) for m < ceil(len P / Q), x zero outside [0, len), in float64, and
    A[m] = sum_n |x[n]| |s h(...)|.  Every n at which h can be non-zero is visited (|m Q / P - n| < Z / s)."""
    x = np.asarray(x, dtype=np.float64)
    P, Q = ratio(sr_in, sr_out)
    s = min(1.0, P / Q)
    reach = half_width(P, Q) + 1
    m = np.arange(-(-len(x) * P // Q), dtype=np.int64)
    n = (m * Q // P)[:, None] + np.arange(-reach, reach + 2, dtype=np.int64)[None, :]
    coef = s * h(s * (m[:, None] * Q - n * P) / P)
    xn = np.where((n >= 0) & (n < len(x)), x[np.clip(n, 0, len(x) - 1)], 0.0)
    return (xn * coef).sum(axis=1), (np.abs(xn) * np.abs(coef)).sum(axis=1)


def trim64(y, top_db=20.0, frame_length=2048, hop=512):
    """librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) in float64: ((start, end), the smallest
    |dB[t] + top_db| over the frames: how far the nearest frame is from the threshold)."""
    y = np.asarray(y, dtype=np.float64)
    assert len(y) > frame_length // 2
    p = np.pad(y, frame_length // 2, mode="reflect")
    T = 1 + len(y) // hop
    mse = np.array([np.mean(p[t * hop:t * hop + frame_length] ** 2) for t in range(T)])
    db = 10 * np.log10(np.maximum(1e-10, mse)) - 10 * np.log10(np.maximum(1e-10, mse.max()))
    loud = np.flatnonzero(db > -top_db)
    margin = float(np.abs(db + top_db).min())
    if not len(loud):
        return (0, 0), margin
    return (int(loud[0]) * hop, min(len(y), (int(loud[-1]) + 1) * hop)), margin
