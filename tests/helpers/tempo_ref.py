"""Restatements of include/nsg.h's nsg_audio_tempo (waveform-similarity overlap-add) and nsg_audio_mix_noise in numpy: the fp32
ones operation for operation, every step rounded to fp32 in the header's order, so that the kernels can be held to them bit for
bit; the fp64 ones for what the fp32 arithmetic costs.  Nothing here imports the package."""
import math

import numpy as np

MIX_PARTIAL = 4096                   # include/nsg.h: NSG_MIX_PARTIAL


def out_length(n, factor):
    """floor(n / factor) in fp64: the samples a clip of n has after a tempo change by factor."""
    return int(np.floor(np.float64(n) / np.float64(factor)))


def _wsola(x, n, factor, S, O, W, L_out, dt):
    x = np.asarray(x)
    n = len(x) if n is None else int(n)
    Ho = S - O
    out_len = out_length(n, factor)
    L_out = out_len if L_out is None else int(L_out)
    out_len = min(out_len, L_out)
    M, M_max = -(-out_len // Ho), -(-L_out // Ho)
    xz = np.zeros(n + 2 * S + 2 * W + O, dtype=dt)                  # x, zero outside [0, n); samples past n are not looked at
    xz[:n] = x[:n]
    q = np.full(M_max, -1, dtype=np.int32)
    out = np.zeros(L_out, dtype=dt)
    ramp = (np.arange(O, dtype=np.float32) / np.float32(O)).astype(dt) if dt == np.float32 else np.arange(O, dtype=dt) / dt(O)
    for m in range(M):
        if m == 0:
            q[0] = 0
        else:
            p = np.float64(m * Ho) * np.float64(factor)            # one fp64 product
            nm = int(p) if 0.0 <= p < n else n
            tail = xz[q[m - 1] + Ho:q[m - 1] + Ho + O]
            d = np.zeros(W, dtype=dt)                               # one chain per delta, j ascending, from +0.0
            for j in range(O):
                t = tail[j] - xz[nm + j:nm + j + W]
                sq = t * t
                d = d + sq
            q[m] = nm + int(np.argmin(d))                           # the first minimum
        k0 = m * Ho
        cnt = min(Ho, out_len - k0)
        seg = xz[q[m]:q[m] + cnt].copy()
        if m >= 1:
            c = min(O, cnt)
            a, b = xz[q[m - 1] + Ho:q[m - 1] + Ho + c], seg[:c]
            diff = b - a
            sc = ramp[:c] * diff
            seg[:c] = a + sc
        out[k0:k0 + cnt] = seg
    return out, out_len, q


def wsola_f32(x, n=None, factor=1.0, S=1808, O=265, W=324, L_out=None):
    """nsg_audio_tempo for one clip, x[:n] (n None: all of x), every operation rounded to fp32 -> (out (L_out,) float32 with +0.0
    past out_len, out_len, positions (ceil(L_out / Ho),) int32 with -1 past the clip's segments).  L_out None: out_len."""
    x = np.asarray(x, dtype=np.float32)
    out, out_len, q = _wsola(x, n, factor, S, O, W, L_out, np.float32)
    assert out.dtype == np.float32
    return out, out_len, q


def wsola_f64(x, n=None, factor=1.0, S=1808, O=265, W=324, L_out=None):
    """The same definition in fp64 throughout."""
    return _wsola(np.asarray(x, dtype=np.float64), n, factor, S, O, W, L_out, np.float64)


def _chain(parts):
    """0.0 + parts[0] + parts[1] + ... in that order (fp64); parts: a sequence of equal-shaped arrays or numbers."""
    t = np.zeros_like(np.asarray(parts[0], dtype=np.float64))
    for p in parts:
        t = t + p
    return t


def energy_in_order(v):
    """sum (double)v_i^2 in nsg_audio_mix_noise's order: partials of 4096 samples -- thread t of 256 adds the squares of samples
    t + 256 k, k = 0 .. 15, to 0.0, then nsg_block_sum_four_walk over the 256 thread sums -- closed by nsg_wave_close_sum."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    if len(v) == 0:
        return 0.0
    NP = -(-len(v) // MIX_PARTIAL)
    sq = np.zeros(NP * MIX_PARTIAL)
    sq[:len(v)] = v * v                                             # exact: 24-bit significands
    sq = sq.reshape(NP, MIX_PARTIAL // 256, 256)                    # [p][k][t]  (a skipped sample and an added +0.0 give the same sum)
    T = _chain([sq[:, k] for k in range(MIX_PARTIAL // 256)])       # (NP, 256) thread sums
    u = ((T[:, :64] + T[:, 64:128]) + T[:, 128:192]) + T[:, 192:]
    part = _chain([u[:, t] for t in range(64)])                     # (NP,)
    lanes = np.zeros(-(-NP // 64) * 64)
    lanes[:NP] = part
    lane_sums = _chain(list(lanes.reshape(-1, 64)))                 # lane l: partials l, l + 64, ...
    return float(_chain(list(lane_sums)))


def _noise_under(noise, offset, n):
    return np.asarray(noise)[(int(offset) + np.arange(n, dtype=np.int64)) % len(noise)]


def mix_f32(x, n, noise, gain, level, offset, L=None):
    """nsg_audio_mix_noise for one clip x[:n] -> (out (L,) float32, +0.0 past n; E_x; E_n; s float32)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x) if n is None else int(n)
    L = len(x) if L is None else int(L)
    v = _noise_under(np.asarray(noise, dtype=np.float32), offset, n)
    ex, en = energy_in_order(x[:n]), energy_in_order(v)
    s = np.float32(0.0)
    if n > 0 and en != 0.0:
        s = np.float32(np.float64(np.float32(level)) * np.sqrt(np.float64(ex) / np.float64(en)))
    out = np.zeros(L, dtype=np.float32)
    gx = np.float32(gain) * x[:n]
    sv = s * v
    out[:n] = gx + sv
    return out, ex, en, s


def mix_f64(x, n, noise, gain, level, offset, L=None):
    """The same definition in fp64, the energies by math.fsum -> (out (L,) float64, E_x, E_n, s)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x) if n is None else int(n)
    L = len(x) if L is None else int(L)
    v = _noise_under(np.asarray(noise, dtype=np.float64), offset, n)
    ex, en = math.fsum(x[:n] * x[:n]), math.fsum(v * v)
    s = float(level) * math.sqrt(ex / en) if n > 0 and en != 0.0 else 0.0
    out = np.zeros(L)
    out[:n] = float(gain) * x[:n] + s * v
    return out, ex, en, s
