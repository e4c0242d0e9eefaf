"""References and case tables of the resampler's and the silence trimmer's envelope tests (tests/test_gpu_resample_trim_envelope.py
runs the kernels of csrc/resample.hip on them, tests/test_resample_envelope_host.py checks on the CPU what they assume).  Nothing
here is computed from a kernel's output: the exact probes are integer arithmetic in int64, the frame energies float64 on
resample64.trim64's padding, the bounds trim64's own, and every case that is held to exact bounds is built so that the float64
reference alone is at least MARGIN_DB from the threshold."""
import functools

import numpy as np

from tests.helpers import resample64 as R

U32 = 2.0 ** -24                              # unit roundoff of fp32
TILE = 256                                    # csrc/resample.hip RS_TILE: outputs per workgroup
LDS_FLOATS = 64 * 1024 // 4                   # RS_MAX_LDS in floats
MARGIN_DB = 0.01                              # tests/test_gpu_resample_trim.py's condition for exact bounds


def out_len(n, P, Q):
    return -(-int(n) * P // Q)


def span_floats(P, Q, W):
    """include/nsg.h: a tile's input span, 255 Q / P + 2 W + 1 floats."""
    return (TILE - 1) * Q // P + 2 * W + 1


def kernel_layout(c, Q):
    """c (P, 2W) phase-major -> the kernel's (2W, P): tap-major, column k holding phase (k Q) mod P (audio._resample_table_on)."""
    P = c.shape[0]
    return np.ascontiguousarray(c[(np.arange(P) * Q) % P].T)


# ----------------------------------------------------------------------------------------------------------------------
# the resampler's exact index probe
# ----------------------------------------------------------------------------------------------------------------------
# (P, Q, W, L_in).  L_out = ceil(L_in P / Q): 1050, 800, 700, 600, 603, 320, 300 -- none a multiple of 256, so each has a tail tile.
PROBE_GEOMETRIES = [(3, 2, 2, 700), (2, 3, 3, 1200), (7, 5, 1, 500), (1, 1, 1, 600), (257, 256, 2, 600), (64, 1, 2, 5), (1, 64, 31, 64 * 300)]
PROBE_MAX = 8                                 # samples and coefficients are integers in [-8, 8]


def probe_lengths(P, Q, W, L_in):
    """0, 1, W - 1, W, L_in, the two lengths whose outputs end either side of the first tile boundary (ceil(a P / Q) <= 256 <
    ceil((a + 1) P / Q)), and one whose outputs end inside a tile that is not the last, so that a whole tile lies past it."""
    a = TILE * Q // P
    assert out_len(a, P, Q) <= TILE < out_len(a + 1, P, Q) and a + 1 <= L_in
    tiles = -(-out_len(L_in, P, Q) // TILE)
    inner = max(1, (TILE * max(tiles - 2, 0) + 100) * Q // P)
    assert -(-out_len(inner, P, Q) // TILE) < tiles
    return [0, 1, W - 1, W, L_in, a, a + 1, inner]


def probe_tables(P, Q, W):
    """Two (P, 2W) int64 tables: seeded entries in [-8, 8], and pairwise distinct entries 1 + phase 2W + tap (at most 1028)."""
    rs = np.random.RandomState(1000 * P + 10 * Q + W)
    return rs.randint(-PROBE_MAX, PROBE_MAX + 1, (P, 2 * W)).astype(np.int64), 1 + np.arange(P * 2 * W, dtype=np.int64).reshape(P, 2 * W)


def probe_samples(P, Q, W, L_in):
    """(B, L_in) int64 in [-8, 8], one row per probe length; a clip's first and last sample are not zero."""
    lens = probe_lengths(P, Q, W, L_in)
    rs = np.random.RandomState(7 * P + 3 * Q + W)
    x = rs.randint(-PROBE_MAX, PROBE_MAX + 1, (len(lens), L_in)).astype(np.int64)
    for b, n in enumerate(lens):
        if n:
            x[b, 0], x[b, n - 1] = 5 + b % 3, -(3 + b % 5)
    return x


def impulse_comb(W, L_in):
    """Unit impulses 2W apart, the first at W - 1: every run of 2W consecutive samples holds exactly one, so with the distinct
    table an output inside the clip is the one entry c[phase][tap] it used (or 0 where that impulse lies outside the clip)."""
    x = np.zeros(L_in, dtype=np.int64)
    x[W - 1::2 * W] = 1
    return x


def probe_ref(x, n, c, P, Q, W, L_out):
    """include/nsg.h's formula in int64: out[m] = sum_j x[floor(m Q / P) - W + 1 + j] c[(m Q) mod P][j] for m < ceil(n P / Q),
    x zero outside [0, n); zeros up to L_out.  Also the largest magnitude any partial sum reaches (in tap order)."""
    out = np.zeros(L_out, dtype=np.int64)
    m = np.arange(out_len(n, P, Q), dtype=np.int64)          # the loop over m, taken at once; the loop over j below
    acc = np.zeros(len(m), dtype=np.int64)
    top = 0
    for j in range(2 * W):
        at = m * Q // P - W + 1 + j
        live = (at >= 0) & (at < n)
        acc += np.where(live, x[np.clip(at, 0, max(n - 1, 0))] * c[(m * Q) % P, j], 0)
        top = max(top, int(np.abs(acc).max(initial=0)))
    out[:len(m)] = acc
    return out, top


# ----------------------------------------------------------------------------------------------------------------------
# production tables: the rates of tests/test_gpu_resample_trim.py and audio.pitch_shift's ratios as (orig_sr, target_sr)
# ----------------------------------------------------------------------------------------------------------------------
RATES = [(16000, 22050), (48000, 22050), (44100, 22050), (11025, 22050), (22050, 16000)]
PITCH_RATIOS = [(196, 185), (185, 196), (3, 2), (2, 3)]      # pitch_shift(num, den) resamples with orig_sr = num, target_sr = den


def production_lengths(sr_in, sr_out):
    """tests/test_gpu_resample_trim.py's lengths_for: shorter than the half width, 3001, and either side of the first tile boundary."""
    P, Q = R.ratio(sr_in, sr_out)
    a = TILE * Q // P
    assert out_len(a, P, Q) <= TILE < out_len(a + 1, P, Q)
    return [50, 3001, a, a + 1]


@functools.lru_cache(maxsize=None)
def production_case(sr_in, sr_out):
    """(clips, [(y64, A)]): uniform noise in [-1, 1) at production_lengths and its fp64 resampling, computed once."""
    clips, refs = [], []
    for n in production_lengths(sr_in, sr_out):
        x = np.random.RandomState(n).uniform(-1, 1, n).astype(np.float32)
        y, A = R.resample64(x, sr_in, sr_out)
        for a in (x, y, A):
            a.setflags(write=False)
        clips.append(x)
        refs.append((y, A))
    return clips, refs


def resample_bound(sr_in, sr_out, A):
    """tests/test_gpu_resample_trim.py's bound: one rounding per coefficient and one per fmaf of the 2W-term chain, each at most
    2^-24 of the sum of the terms' magnitudes."""
    P, Q = R.ratio(sr_in, sr_out)
    return (2 * R.half_width(P, Q) + 2) * U32 * A + 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# frame energies
# ----------------------------------------------------------------------------------------------------------------------
ENERGY_FRAMES = (2, 62, 64, 66, 2048, 8192)
ENERGY_TARGET = {2: 300, 62: 300, 64: 300, 66: 300, 2048: 1100, 8192: 4200}      # about how long the longer clips are: L stays small


def energy_hops(N):
    return sorted({1, 7, max(1, N // 4), 2 * N})             # 2N leaves gaps between the frames


def energy_lengths(N, hop):
    """The shortest legal clip N/2 + 1, a multiple of hop and one more than it (the frame count 1 + len / hop steps there)."""
    m = max(-(-(N // 2 + 2) // hop), -(-ENERGY_TARGET[N] // hop))
    return [N // 2 + 1, m * hop, m * hop + 1]


def energy_clips(N, hop):
    """Noise that is loud at both ends of every clip (0.3 sigma, scaled per clip), so that both reflect folds carry weight."""
    rs = np.random.RandomState(N + 31 * hop)
    return [((0.2 + 0.4 * i) * 0.3 * rs.randn(n)).astype(np.float32) for i, n in enumerate(energy_lengths(N, hop))]


def frame_mse64(y, N, hop):
    """mean(p[t hop : t hop + N]^2) for t < 1 + len / hop on trim64's padding p = reflect_pad(y, N/2), float64 (or, for an
    integer y, the int64 sums of squares: exact)."""
    y = np.asarray(y)
    exact = np.issubdtype(y.dtype, np.integer)
    p = np.pad(y.astype(np.int64 if exact else np.float64), N // 2, mode="reflect")
    sq = np.lib.stride_tricks.sliding_window_view(p * p, N)[::hop][:1 + len(y) // hop]
    out = np.empty(len(sq), dtype=sq.dtype)
    for t0 in range(0, len(sq), 256):
        out[t0:t0 + 256] = sq[t0:t0 + 256].sum(axis=1) if exact else sq[t0:t0 + 256].mean(axis=1)
    return out


def energy_bound(N, mse):
    """A lane's chain of at most ceil(N / 64) fmaf roundings, six butterfly adds and one division, each at most 2^-24 of a partial
    sum; every term is non-negative, so a partial sum is at most the sum itself: (ceil(N / 64) + 8) 2^-24 mse."""
    return (-(-N // 64) + 8) * U32 * mse


# (N, hop) of the exact probe: N a power of two, integer samples in [-3, 3], so a frame's sum of squares is at most 9 N < 2^24
EXACT_ENERGY = [(2, 1), (64, 16), (64, 7), (2048, 512), (8192, 2048), (8192, 130)]
EXACT_MAX = 3


def exact_energy_clips(N, hop):
    """Integer clips at energy_lengths(N, hop) whose first and last three samples have the squares 9, 4, 1: a fold that is off by
    one sample, or repeats the edge, changes the sum."""
    rs = np.random.RandomState(5 * N + hop)
    clips = []
    for n in energy_lengths(N, hop):
        y = rs.randint(-EXACT_MAX, EXACT_MAX + 1, n).astype(np.int64)
        edge = np.array([3, -2, 1])[:min(3, n // 2)]
        y[:len(edge)], y[n - len(edge):] = edge, -edge[::-1]
        clips.append(y)
    return clips


# ----------------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------------
HOP = 16                                      # of every bounds case; with frame_length 16 the frames tile the clip without overlap
LOUD, QUIET = 0.5, 1e-4
FLOOR_AMP = float(np.sqrt(1e-9))              # a frame of this amplitude has mse 1e-9, 10 dB above the 1e-10 floor
# (frame_length, hop, top_db) of the launches; a clip no longer than frame_length / 2 is left out of a launch
BOUNDS_LAUNCHES = [(16, HOP, 20.0), (16, HOP, 5.0), (16, HOP, 0.5), (16, HOP, 200.0), (64, HOP, 20.0), (64, HOP, 5.0)]


def _signs(n, seed):
    return np.random.RandomState(seed).choice([-1.0, 1.0], n)


def _levels(T, r, spans, seed, rest=QUIET):
    """A clip of (T - 1) HOP + r samples, T frames: samples of constant magnitude and seeded sign, `rest` everywhere but the
    spans (first frame, last frame, amplitude), which cover exactly those frames of the (16, 16) grid, [16 f - 8, 16 l + 8)."""
    n = (T - 1) * HOP + r
    y = rest * np.ones(n)
    for first, last, amp in spans:
        y[max(0, HOP * first - HOP // 2):HOP * last + HOP // 2] = amp
    return (y * _signs(n, seed)).astype(np.float32)


def _db(d):
    return LOUD * 10.0 ** (d / 20.0)


@functools.lru_cache(maxsize=None)
def bounds_clips():
    """name -> (clip, {top_db: (first, last) non-silent frame at (16, 16)} where the case is about them).  Frame counts 1, 63, 64,
    65, 255, 256, 257 and 513; first or last non-silent frames on 63 | 64 (a wave of trim_bounds_kernel) and 255 | 256 | 257 (a
    round of it)."""
    c = {}
    for name, T, r, first, last in (("T1", 1, 11, 0, 0), ("T63_only_frame_0", 63, 3, 0, 0), ("T64_only_the_last", 64, 5, 63, 63),
                                    ("T65_only_the_last", 65, 5, 64, 64), ("T255_63_to_64", 255, 9, 63, 64),
                                    ("T256_only_the_last_no_remainder", 256, 0, 255, 255), ("T257_64_to_the_last", 257, 1, 64, 256),
                                    ("T513_255_to_257", 513, 7, 255, 257), ("T513_257_to_the_last", 513, 0, 257, 512),
                                    ("T300_only_256", 300, 2, 256, 256), ("T300_0_to_63", 300, 15, 0, 63)):
        c[name] = (_levels(T, r, [(first, last, LOUD)], len(c)), {td: (first, last) for td in (20.0, 5.0, 0.5)})
    c["all_zeros"] = (np.zeros(777, dtype=np.float32), {})
    c["below_the_floor"] = ((1e-6 * _signs(500, 50)).astype(np.float32), {})          # mse 1e-12 everywhere
    # mse 1e-9 beside exactly silent frames: the floor holds those 10 dB down, so 20 dB keeps every frame and 5 dB the loud ones
    c["floor"] = (_levels(30, 4, [(8, 12, FLOOR_AMP), (20, 21, FLOOR_AMP)], 51, rest=0.0), {20.0: (0, 29), 5.0: (8, 21), 0.5: (8, 21), 200.0: (0, 29)})
    # the loudest frames, frames 0.3 dB below them and frames 0.7 dB below them: 0.5 dB separates the last two
    steps = [(5, 9, _db(-0.7)), (10, 19, LOUD), (20, 24, _db(-0.3)), (25, 29, _db(-0.7))]
    c["steps"] = (_levels(40, 6, steps, 52), {0.5: (10, 24), 5.0: (5, 29), 20.0: (5, 29), 200.0: (0, 39)})
    c["steps_from_frame_0"] = (_levels(270, 0, [(0, 3, _db(-0.3)), (4, 200, _db(-0.7)), (201, 255, LOUD), (256, 256, _db(-0.3)), (257, 260, _db(-0.7))], 53),
                               {0.5: (0, 256), 5.0: (0, 260)})
    for y, _ in c.values():
        y.setflags(write=False)
    return c


def bounds_launch(frame_length):
    """(names, clips) of a launch at this frame_length: every clip longer than frame_length / 2."""
    names = [k for k, (y, _) in bounds_clips().items() if len(y) > frame_length // 2]
    return names, [bounds_clips()[k][0] for k in names]


@functools.lru_cache(maxsize=None)
def bounds_ref(name, frame_length, hop, top_db):
    """trim64 of a clip: ((start, end), margin), computed once."""
    return R.trim64(bounds_clips()[name][0], top_db, frame_length, hop)
