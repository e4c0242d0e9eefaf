"""What tests/test_gpu_psola_envelope.py launches and tests/test_psola_envelope_host.py proves sound: the case table over the
launch constants of nsg_audio_pitch_marks / nsg_audio_psola, cheap signals, a simulation of psola_marks_kernel's ring rule over
the searches the restatement records, and closed forms for the marks of a ramp.  numpy only; no kernel, no torch."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.helpers import psola_ref as R

PS_H = 4096                                            # csrc/psola.hip: samples of a ring half
PS_FR = 1024                                           # period slots
PS_TILE = 1024                                         # output samples of an overlap-add block

Geo = namedtuple("Geo", "hop sr P_u P_min P_max alpha")
DEFAULT = Geo(256, 22050, 110, 45, 339, (1, 4))
WIDE = Geo(256, 22050, 1024, 2, 1024, (1, 2))          # the longest period, the widest search: ramps at P = 1024
STRESS = Geo(16, 22050, 1024, 2, 1024, (1, 2))

# name, n, geometry, f0 Hz, share of unvoiced frames, T (None: 1 + n // hop), ratio
Case = namedtuple("Case", "name n geo f0 unvoiced T ratio")
CASES = [
    Case("widest", 20000, Geo(256, 22050, 700, 512, 1024, (1, 2)), 25.0, 0.15, None, 1.3),
    Case("narrowest", 6000, Geo(16, 8000, 1, 2, 8, (1, 2)), 2000.0, 0.0, None, 0.5),
    Case("alpha zero", 20000, Geo(256, 22050, 110, 45, 339, (0, 1)), 150.0, 0.0, None, 2.0),
    Case("big denominator", 20000, Geo(64, 22050, 110, 45, 339, (262143, 1 << 20)), 150.0, 0.0, None, 0.8),
    Case("small hop", 40000, Geo(16, 22050, 110, 45, 339, (1, 4)), 150.0, 0.0, None, 1.25),
    Case("long", 300000, DEFAULT, 150.0, 0.0, None, 1.25),
    Case("one frame for all", 20000, Geo(1 << 20, 22050, 110, 45, 339, (1, 4)), 150.0, 0.0, None, 4.0),
    Case("T = 1", 20000, DEFAULT, 150.0, 0.0, 1, 0.25),
    Case("short track", 20000, DEFAULT, 150.0, 0.0, 20, 1.25),
    Case("P_u above", 20000, Geo(256, 22050, 5000, 45, 339, (1, 4)), 150.0, 1.0, None, 1.0),
]
BY_NAME = {c.name: c for c in CASES}
SMALL = Case("small", 6000, DEFAULT, 150.0, 0.0, None, 1.25)          # the clip the hostile marks and the relaunches start from

# (f0_in, f0_out) of a frame, fp32: the ratio exactly 0.25 and 4; its float32 neighbours outside and inside; 2 / 3 and 2, which put
# D / r + 0.5 on an integer for D = 147 (the host test checks each of these statements in fp64)
EDGE_N = 40 * 147 + 1                                  # pulses(EDGE_N, 147): the last pulse is the last sample
_f = np.float32
RATIO_EDGES = [(_f(150), _f(37.5)), (_f(150), _f(600)), (_f(150), np.nextafter(_f(37.5), _f(0))), (_f(150), np.nextafter(_f(600), _f(1e9))),
               (_f(150), np.nextafter(_f(37.5), _f(1e9))), (_f(150), np.nextafter(_f(600), _f(0))), (_f(150), _f(100)), (_f(150), _f(300))]


def pulses(n, P, seed=7):
    """A unit pulse every P samples from 0 over noise of 1e-3: under a track of period P the marks are the pulses, D = P."""
    x = 1e-3 * np.random.default_rng(seed).standard_normal(n)
    x[::P] = 1.0
    return x.astype(np.float32)


def edge_tracks(n, geo, run=3):
    """Tracks whose frames walk through RATIO_EDGES, `run` frames each -> (f0_in, f0_out)."""
    T = 1 + n // geo.hop
    pick = (np.arange(T) // run) % len(RATIO_EDGES)
    return (np.array([RATIO_EDGES[i][0] for i in pick], dtype=np.float32), np.array([RATIO_EDGES[i][1] for i in pick], dtype=np.float32))


def harmonic(n, f0, sr, seed=0, amp=0.5, noise=0.02):
    """A sum of the harmonics of f0 below sr / 2 (at most six, amplitudes 0.6^h, fixed random phases) plus white noise, normalised
    to `amp` -> (n,) float32.  One maximum per period, vectorised: 300 000 samples in milliseconds."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = noise * rng.standard_normal(n)
    for h in range(1, 7):
        if h * f0 < 0.5 * sr:
            x += 0.6 ** h * np.sin(2.0 * np.pi * h * f0 * t / sr + (rng.uniform(0.0, 2.0 * np.pi) if h > 1 else 0.0))
    peak = np.abs(x).max() if n else 0.0
    return (x * (amp / peak if peak > 0 else 1.0)).astype(np.float32)


def ramp(n, sign=1):
    """x[i] = sign i 2^-17: exact in fp32 for i < 2^24, strictly monotone, so the maximum of a range is its last (first) sample."""
    assert n < 1 << 24
    return (sign * np.arange(n, dtype=np.float64) * 2.0 ** -17).astype(np.float32)


def constant_track(n, geo, P):
    """An all-voiced track whose every frame has the period P: sr / P Hz in fp32 (the host test checks that it rounds back to P)."""
    return np.full(1 + n // geo.hop, np.float32(geo.sr / P), dtype=np.float32)


def build(case):
    """A case's clip and tracks -> (x (n,) float32, f0_in (T,), f0_out (T,))."""
    g = case.geo
    seed = {c.name: i for i, c in enumerate(CASES)}.get(case.name, len(CASES))
    x = harmonic(case.n, case.f0, g.sr, seed=seed)
    T = 1 + case.n // g.hop if case.T is None else case.T
    f = np.full(T, case.f0, dtype=np.float32)
    if case.unvoiced > 0:
        f[np.random.default_rng(100 + seed).random(T) < case.unvoiced] = 0.0
    return x, f, (f * np.float32(case.ratio)).astype(np.float32)


def stress():
    """The ring-stress case: a rising ramp of 60 000 samples at hop 16, periods [2, 1024], alpha 1/2, P_u = 1024, every frame
    voiced with the period 1024 or unvoiced by a fair coin -> (x, f0_in)."""
    n = 60000
    f = constant_track(n, STRESS, 1024)
    f[np.random.default_rng(0).random(len(f)) >= 0.5] = 0.0
    return ramp(n), f


def seam():
    """The frame two ring halves share.  At hop 16 half h holds the frames 256 h .. 256 (h + 1), so a commit of half h + 2 writes
    frame 256 (h + 3) while frame 256 (h + 1) -- the first of the older live half, 512 slots away -- can still be read: by a mark in
    the first eight samples of half h + 1, found by the very search that set off the commit.  A falling ramp of 16 000 samples,
    all unvoiced at P_u = 1024 but for frame 256 (P = 512): the marks 0, 1024, .. reach 4096 exactly, the search for it commits
    half 2 (frames 512 .. 768), and the next period read is frame 256's, which differs from frame 768's -> (x, f0_in)."""
    n = 16000
    f = np.zeros(1 + n // STRESS.hop, dtype=np.float32)
    f[PS_H // STRESS.hop] = np.float32(STRESS.sr / 512)
    return ramp(n, -1), f


def reference(x, n, f0_in, f0_out, geo, dtype=np.float32, J_max=None, H_max=None, marks=None, clamps=None):
    """R.psola_ref under a geometry; `marks` (with clamps = (n_marks, K_max)) in place of the clip's own marks."""
    n = max(0, min(int(n), len(x)))
    if marks is None:
        marks = R.marks_ref(x, n, f0_in, geo.hop, geo.sr, geo.P_u, geo.P_min, geo.P_max, geo.alpha)
    else:
        marks = R.clamped_marks(marks, clamps[0], clamps[1], n)
    syn, mp = R.syn_ref(marks, f0_in, f0_out, geo.hop, geo.P_u, geo.P_min, geo.P_max, J_max=J_max)
    out, den, cnt = R.ola_ref(x, n, marks, syn, mp, dtype, H_max=H_max)
    return dict(marks=marks, syn=syn, map=mp, out=out, den=den, grains=cnt)


def ring_walk(marks, searches, hop, T):
    """psola_marks_kernel's ring rule over the searches R.marks_trace recorded: the live halves are base, base + 1; a search whose
    range starts in half base + 1 (lo >= (base + 1) PS_H) commits half base + 2 after it -> dict(step: the largest lo - previous
    lo (the first range starts at 0), reach: the deepest hi - (base + 1) PS_H of a voiced search, advances, frame: the highest
    frame whose period is read, inside: every range within the two live halves)."""
    base, prev, step, reach, inside = 0, 0, 0, -(1 << 62), True
    for lo, hi, P in searches:
        inside = inside and lo >= base * PS_H and hi < (base + 2) * PS_H
        step, prev = max(step, lo - prev), lo
        if P > 0:
            reach = max(reach, hi - (base + 1) * PS_H)
        if lo >= (base + 1) * PS_H:
            base += 1
    top = max((R.frame(m, hop, T) for m in marks), default=-1)
    return dict(step=step, reach=reach, advances=base, frame=top, inside=inside)


def rising_marks(n, P, alpha):
    """The marks of ramp(n) under an all-voiced track of constant period P: every search takes its range's last sample."""
    d = alpha[0] * P // alpha[1]
    m = [min(P, n) - 1]
    while m[-1] + P - d <= n - 1:
        m.append(min(m[-1] + P + d, n - 1))
    return m


def falling_marks(n, P, alpha):
    """... of ramp(n, -1): every search takes its range's first sample."""
    d = alpha[0] * P // alpha[1]
    return list(range(0, n, P - d))


# hostile (marks, n_marks) for nsg_audio_psola, from a clip's true marks row (K_max,) int32 and count: name -> (row, count)
def hostile(marks, K, K_max, n):
    row = np.asarray(marks, dtype=np.int32)
    out = {}
    for name, count in (("count -5", -5), ("count 0", 0), ("count above K_max", K_max + 9)):
        out[name] = (row.copy(), count)
    neg, big, past, rev, rep = (row.copy() for _ in range(5))
    neg[2:K:5] = -7
    big[3:K:7] = 2 ** 31 - 1
    past[K // 2:K:3] = n
    past[K // 2 + 1:K:3] = n + 12345
    rev[K // 4:K // 2] = rev[K // 4:K // 2][::-1].copy()
    rep[K // 3:K // 3 + 6] = rep[K // 3]
    rep[K - 4:K] = rep[K - 4]
    for name, r in (("-7", neg), ("2^31 - 1", big), (">= len", past), ("a reversed run", rev), ("repeats", rep)):
        out[name] = (r, K)
    return out
