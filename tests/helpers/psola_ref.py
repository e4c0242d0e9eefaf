"""Restatements of include/nsg.h's nsg_audio_pitch_marks and nsg_audio_psola (time-domain pitch-synchronous overlap-add) in
numpy, one clip at a time: the marks, synthesis marks and mapping are integers and have one statement; the overlap-add has two,
fp32 in the header's operation order (what the kernel must equal bit for bit) and fp64 (what it must be close to, with the bound
derived below from the roundings, not from a run).  And the synthetic vowel the tests use.  numpy only; no kernel, no torch."""
from __future__ import annotations

import math

import numpy as np

EPS32 = 2.0 ** -24                                     # half an ulp of 1: the relative error of one fp32 rounding
MIN_WEIGHT = 2.0 ** -10                                # NSG_PSOLA_MIN_WEIGHT_LOG2
ALPHA = (1, 4)


def sizes(L, P_min, P_max, alpha=ALPHA):
    """(G, K_max, H_max, G_s, J_max) as include/nsg.h defines them."""
    an, ad = alpha
    G = P_min - an * P_min // ad
    Gs = max(1, int(math.floor(G / 4.0 + 0.5)))
    return G, -(-L // G), P_max + an * P_max // ad, Gs, -(-L // Gs)


def clamp(p, lo, hi):
    return lo if not p >= lo else (hi if p > hi else p)


def frame(n, hop, T):
    return min(T - 1, (n + hop // 2) // hop)


def period(f, sr, P_u, P_min, P_max):
    """The signed period of a frame whose track value is f (fp32): + P voiced, - clamp(P_u) unvoiced."""
    f = np.float32(f)
    if not f > 0:
        return -clamp(P_u, P_min, P_max)
    with np.errstate(all="ignore"):
        v = np.floor(np.float64(np.float32(sr)) / np.float64(f) + 0.5)
    if not v >= P_min:
        return P_min
    if v > P_max:
        return P_max
    return int(v)


def argmax_key(x, lo, hi):
    """The index of the greatest key over x[lo .. hi] (fp32): the order of the reals on the bits, the smallest index of equals."""
    u = np.ascontiguousarray(x[lo:hi + 1], dtype=np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(u >> np.uint64(31), u ^ np.uint64(0xffffffff), u ^ np.uint64(0x80000000))
    key = (o << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(hi - lo + 1, dtype=np.uint64))
    return lo + int(np.argmax(key))


def marks_trace(x, n, f0, hop, sr, P_u, P_min, P_max, alpha=ALPHA):
    """marks_ref, and every search after the first one as the chain made it -> (marks, [(lo, hi, P)]): the range of search k + 1
    and the signed period it was derived from (lo = hi and P < 0 from an unvoiced frame), the search that ended the chain with
    lo > n - 1 left out, as the kernel leaves it before it touches its ring."""
    n = max(0, min(int(n), len(x)))
    if n == 0:
        return [], []
    T, (an, ad) = len(f0), alpha
    per = lambda s: period(f0[frame(s, hop, T)], sr, P_u, P_min, P_max)
    m = argmax_key(x, 0, min(abs(per(0)), n) - 1)
    marks, searches = [m], []
    while True:
        pp = per(m)
        if pp > 0:
            d = an * pp // ad
            lo, hi = m + pp - d, min(m + pp + d, n - 1)
        else:
            lo = hi = m - pp
        if lo > n - 1:
            return marks, searches
        searches.append((lo, hi, pp))
        m = argmax_key(x, lo, hi) if pp > 0 else lo
        marks.append(m)


def marks_ref(x, n, f0, hop, sr, P_u, P_min, P_max, alpha=ALPHA):
    """nsg_audio_pitch_marks for one clip x[:n] with the track f0 (T,) -> the marks, a list of ints."""
    return marks_trace(x, n, f0, hop, sr, P_u, P_min, P_max, alpha)[0]


def clamped_marks(marks, n_marks, K_max, n):
    """The marks as nsg_audio_psola reads a row `marks` (at least min(n_marks, K_max) long) and a count it did not make itself:
    K = n_marks clamped into [0, K_max] (0 for an empty clip), every mark clamped into [0, n - 1] -> a list of K ints."""
    K = clamp(int(n_marks), 0, K_max) if n > 0 else 0
    return [clamp(int(m), 0, n - 1) for m in list(marks)[:K]]


def syn_ref(marks, f0_in, f0_out, hop, P_u, P_min, P_max, J_max=None, clamps=None):
    """The synthesis marks and the mapping of nsg_audio_psola for one clip -> (syn, map), lists of ints.  J_max: the chain also
    ends when it holds J_max marks (never reached with nsg_audio_pitch_marks' marks and J_max >= ceil(L / G_s)).  clamps =
    (n_marks, K_max, n): `marks` is a row as handed to the entry point, read through clamped_marks."""
    if clamps is not None:
        marks = clamped_marks(marks, *clamps)
    K = len(marks)
    if K == 0:
        return [], []
    T = len(f0_in)
    s, a, syn, mp = marks[0], 0, [], []
    while True:
        syn.append(s); mp.append(a)
        D = clamp(P_u, P_min, P_max) if K == 1 else (marks[a + 1] - marks[a] if a < K - 1 else marks[a] - marks[a - 1])
        t = frame(s, hop, T)
        vi, vo, r = np.float32(f0_in[t]), np.float32(f0_out[t]), 1.0
        if vi > 0 and vo > 0:
            with np.errstate(all="ignore"):
                r = float(np.float64(vo) / np.float64(vi))
            r = 0.25 if r < 0.25 else (4.0 if r > 4.0 else (r if r == r else 1.0))
        q = math.floor(D / r + 0.5)
        s2 = s + (int(q) if q >= 1.0 else 1)
        if s2 > marks[-1] or (J_max is not None and len(syn) >= J_max):
            return syn, mp
        s = s2
        while a + 1 < K and abs(marks[a + 1] - s) < abs(marks[a] - s):
            a += 1


def ola_ref(x, n, marks, syn, mp, dtype=np.float32, L=None, H_max=None, clamps=None):
    """The overlap-add of nsg_audio_psola for one clip in `dtype` arithmetic, grains added in ascending j, every operation rounded
    -> (out (L,), den (L,), grains (L,) int: how many grains reach each sample).  clamps = (n_marks, K_max, n): `marks` is a row
    as handed to the entry point, read through clamped_marks.  H_max: a grain reaches only |dist| < H_max, the header's walk over
    s_j -- no restriction on nsg_audio_pitch_marks' marks, which are at most H_max apart; it cuts the halves of foreign ones."""
    L = len(x) if L is None else L
    n = max(0, min(int(n), len(x)))
    if clamps is not None:
        marks = clamped_marks(marks, *clamps)
    F = dtype
    xs = np.asarray(x[:n], dtype=np.float32).astype(F)
    num, den, cnt = np.zeros(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=np.int64)
    K = len(marks)
    for s, a in zip(syn, mp):
        ma = marks[a]
        hl = ma - marks[a - 1] if a > 0 else 0
        hr = marks[a + 1] - ma if a < K - 1 else 0
        for side, half in ((-1, hl), (0, 1), (1, hr)):
            if side == 0:
                dist = np.array([0])
                w = np.ones(1, dtype=F)
            else:
                if half < 2:
                    continue
                dist = side * np.arange(1, half)
                u = np.arange(1, half).astype(F) / F(half)
                w = F(1) - (u * u) * (F(3) - F(2) * u)
            at = s + dist
            ok = (at >= 0) & (at < n)
            if H_max is not None:
                ok &= np.abs(dist) < H_max
            at, src, w = at[ok], ma + dist[ok], w[ok]
            num[at] = num[at] + w * xs[src]
            den[at] = den[at] + w
            cnt[at] += 1
    out = np.zeros(L, dtype=F)
    with np.errstate(all="ignore"):
        out[:n] = np.where(den >= F(MIN_WEIGHT), num / den, xs)
    full = lambda v, fill: np.concatenate([v, np.full(L - n, fill, dtype=v.dtype)])
    return out, full(den, 0), full(cnt, 0)


def psola_ref(x, n, f0_in, f0_out, hop, sr, P_u, P_min, P_max, alpha=ALPHA, dtype=np.float32):
    """Both entry points for one clip -> dict(marks, syn, map, out, den, grains)."""
    marks = marks_ref(x, n, f0_in, hop, sr, P_u, P_min, P_max, alpha)
    syn, mp = syn_ref(marks, f0_in, f0_out, hop, P_u, P_min, P_max)
    out, den, cnt = ola_ref(x, n, marks, syn, mp, dtype)
    return dict(marks=marks, syn=syn, map=mp, out=out, den=den, grains=cnt)


def fp32_bound(den64, grains, peak):
    """|fp32 out - fp64 out| per sample, from the roundings alone.  With e = 2^-24 and g grains reaching a sample: u is one
    rounding and w five more on values <= 3, |dw| <= 12 e; a term fl(w x) adds one, and the two chains add g roundings each on
    partial sums <= g peak and <= g: |d num| <= g peak (13 + g) e, |d den| <= g (12 + g) e; the quotient of num / den, |out| <=
    peak, adds one: |d out| <= peak e (g (25 + 2 g) / den + 1).  Doubled for the second-order terms.  Where no grain decides
    (den below the floor) the output is the input: 0."""
    g = grains.astype(np.float64)
    d = np.maximum(np.asarray(den64, dtype=np.float64), MIN_WEIGHT)
    return np.where(np.asarray(den64) >= MIN_WEIGHT, 2.0 * peak * EPS32 * (g * (25.0 + 2.0 * g) / d + 1.0), 0.0)


def vowel(f0, seconds, sr=22050, formant=1000.0, bandwidth=120.0, unvoiced=(), seed=0, amp=0.5):
    """A synthetic vowel: a pulse train at f0 Hz (a number, or one value per sample for a glide) through a fixed two-pole
    resonator at `formant` Hz, with white-noise stretches (start_s, end_s) in `unvoiced` replacing the pulses -> (x (n,) float32
    normalised to `amp`, voiced (n,) bool)."""
    n = int(round(seconds * sr))
    f = np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))
    voiced = np.ones(n, dtype=bool)
    for a, b in unvoiced:
        voiced[int(a * sr):int(b * sr)] = False
    rng = np.random.default_rng(seed)
    e = np.zeros(n)
    phase = 0.0
    for i in range(n):
        phase += f[i] / sr
        if phase >= 1.0:
            phase -= 1.0
            if voiced[i]:
                e[i] = 1.0
    e[~voiced] = 0.05 * rng.standard_normal(int((~voiced).sum()))
    r = math.exp(-math.pi * bandwidth / sr)
    a1, a2 = 2.0 * r * math.cos(2.0 * math.pi * formant / sr), -r * r
    y = np.zeros(n)
    for i in range(n):
        y[i] = e[i] + (a1 * y[i - 1] if i >= 1 else 0.0) + (a2 * y[i - 2] if i >= 2 else 0.0)
    peak = np.abs(y).max()
    return (y * (amp / peak if peak > 0 else 1.0)).astype(np.float32), voiced


def track(voiced, f0, hop, sr=22050):
    """The ideal track of a vowel(): frame t at sample t hop, f0 (a number or per sample) where that sample is voiced, +0.0 where
    it is not -> (1 + n // hop,) float32."""
    n = len(voiced)
    f = np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))
    t = np.minimum(np.arange(1 + n // hop) * hop, n - 1)
    return np.where(voiced[t], f[t], 0.0).astype(np.float32)
