"""The fp64 yardstick of the wav -> mel front end's kernels (csrc/audio.hip: melspectrogram_kernel, preemphasis_kernel;
csrc/resample.hip: resample_kernel, frame_energy_kernel, trim_bounds_kernel), written from the formulas include/nsg.h states as
the entry points' contracts, with EVERY argument the entry points take (tests/helpers/mel_forward64.py fixes them at the
reference's constants and the Slaney basis, whose rows never weight bins 0..5 or the upper 31 % of the spectrum).
tests/test_frontend_ref_host.py holds this file to the older helpers, to its own tables' conditions and to planted errors;
tests/test_gpu_frontend_envelope.py holds the kernels to it.

Three kinds of check.  MEL: every entry in the amplitude domain, check_mel: mel_forward64.check_amplitude's rule with the
spectral peak taken over the two frames a workgroup transforms together instead of over the clip.  EXACT PROBES: integer samples
and an integer coefficient table (resampler), integer samples (frame energies): every product and partial sum is an integer
below 2^24, so fp32 in any order is exact and a kernel must EQUAL the int64 restatement.  ROUNDING: the existing derived bounds
((2W + 2) 2^-24 A for the resampler, two roundings for pre-emphasis).

The launchers' limits are restated as named constants with the source line they mirror; the case tables are DERIVED from them,
so a changed constant moves the cases (or fails the host test's coverage asserts)."""
import types

import numpy as np

from tests.helpers.mel_forward64 import REL

U32 = 2.0 ** -24
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3      # include/nsg.h:45-47
EXACT_SUM = 2 ** 24                                     # the probes' condition

# ---- the kernels' constants ------------------------------------------------------------------------------------------------------
MEL_MAX_ROWS = 128                      # audio.hip:195 MEL_MAX_ROWS: m = tid & 127, two frames x 128 rows = 256 threads
MEL_NFFTS = (512, 1024, 2048)           # audio.hip:393 lg in 9..11
RS_TILE = 256                           # resample.hip:15 outputs per workgroup
RS_MAX_TABLE = 1 << 20                  # resample.hip:16 floats: P * 2W
RS_MAX_LDS = 64 * 1024                  # resample.hip:17 bytes: the staged input span of a tile
TRIM_BLOCK = 256                        # resample.hip:98,107 trim_bounds_kernel: t += 256
TRIM_MAX_FRAME = 8192                   # resample.hip:163 frame_length <= 8192
EW_BLOCKS, EW_THREADS = 4096, 256       # nsg_common.h:129 ew_blocks: grid-strided above 4096 x 256 elements


def cdiv(a, b):
    return -(-a // b)


def rs_lds_bytes(P, Q, W):
    """resample.hip:146: the dynamic LDS of a launch."""
    return ((RS_TILE - 1) * Q // P + 2 * W + 1) * 4


# ==================================================================================================================================
# melspectrogram
# ==================================================================================================================================
DEFAULT_PARAMS = (0.97, -100.0, 20.0, 1.0)
PARAM_SETS = [DEFAULT_PARAMS, (0.0, -80.0, 0.0, 4.0), (-0.5, -100.0, -20.0, 1.0), (1.0, -60.0, 20.0, 0.5)]
LEAK_PARAMS = (0.0, -300.0, 0.0, 1.0)   # quiet beside loud: k = 0 (disjoint frames), a floor of 1e-15 so that any leak an fp32 FFT could make shows


def hann_periodic(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames_of(p, n_fft, hop, Tb):
    """(Tb, n_fft): reflect_pad(p, n_fft/2)[t hop : t hop + n_fft]."""
    pad = np.pad(p, n_fft // 2, mode="reflect")
    return pad[np.arange(Tb)[:, None] * hop + np.arange(n_fft)[None, :]]


def band_matrix(basis, bands):
    """basis with everything outside each row's [first, last] set to zero (float64): what the contract says is summed."""
    basis = np.asarray(basis, dtype=np.float64)
    f = np.arange(basis.shape[1])[None, :]
    return np.where((f >= bands[:, :1]) & (f <= bands[:, 1:]), basis, 0.0)


def floor_amp(min_db):
    """The amplitude floor under the logarithm as the launcher passes it: (float) pow(10, min_db / 20)."""
    return float(np.float32(10.0 ** (float(min_db) / 20.0)))


def normalise(m, min_db, ref_db, max_abs, floor=None):
    S = 20.0 * np.log10(np.maximum(10.0 ** (min_db / 20.0) if floor is None else floor, m)) - ref_db
    return np.clip(max_abs * (S - min_db) / (-min_db), 0.0, max_abs)


def mel64(x, length, basis, bands, n_fft, hop, k, min_db, ref_db, max_abs):
    """x: one row of L float32 samples, the clip its first `length`.  Returns a namespace: out (n_mels, T) with T = 1 + L / hop
    (zeros for t >= Tb = 1 + length / hop), m (n_mels, Tb) mel amplitudes, X (F, Tb) = |rfft| per frame, rows (n_mels,) =
    sum_f |basis| over each band.  All float64; the parameters are used as given (check_mel hands them over at their fp32 values)."""
    L = len(x)
    y = np.asarray(x, dtype=np.float64)[:length]
    assert n_fft // 2 < length <= L
    p = y.copy()
    p[1:] -= k * y[:-1]
    T, Tb = 1 + L // hop, 1 + length // hop
    X = np.abs(np.fft.rfft(frames_of(p, n_fft, hop, Tb) * hann_periodic(n_fft)[None, :], axis=1)).T
    Bm = band_matrix(basis, bands)
    m = Bm @ X
    out = np.zeros((Bm.shape[0], T))
    out[:, :Tb] = normalise(m, min_db, ref_db, max_abs)
    return types.SimpleNamespace(out=out, m=m, X=X, rows=np.abs(Bm).sum(axis=1), T=T, Tb=Tb)


def amplitude_of(out, min_db, ref_db, max_abs):
    """Undo the normalisation: out = max_abs (20 log10 m - ref_db - min_db) / (-min_db).  Returns (m, lo, hi): an output shows m
    only through clip(m, lo, hi), lo = the larger of the amplitude where the value reaches 0 and the floor under the logarithm
    (with ref_db < 0 the floor comes first and the value never reaches 0), hi = the amplitude where it reaches max_abs."""
    min_db, ref_db, max_abs = (float(np.float32(v)) for v in (min_db, ref_db, max_abs))
    m = 10.0 ** ((np.asarray(out, dtype=np.float64) * (-min_db) / max_abs + min_db + ref_db) / 20.0)
    return m, max(10.0 ** ((min_db + ref_db) / 20.0), 10.0 ** (min_db / 20.0)), 10.0 ** (ref_db / 20.0)


def pair_peak(X):
    """(Tb,): max |X| over the two frames 2 (t // 2) and 2 (t // 2) + 1 of the clip (the second may not exist)."""
    peak = X.max(axis=0)
    Tb = len(peak)
    even = np.pad(peak, (0, Tb % 2)).reshape(-1, 2).max(axis=1)
    return np.repeat(even, 2)[:Tb]


def check_mel(out_gpu, x, length, basis, bands, n_fft, hop, k, min_db, ref_db, max_abs, tag="", ref=None, quiet=False):
    """out_gpu (n_mels, T).  Every entry t < Tb: |m_gpu - clip(m_ref)| <= delta + REL clip(m_ref), delta[j, t] = REL peak(t)
    sum_f |basis[j]|, peak(t) the spectral peak of the PAIR of frames the workgroup transforms as one complex FFT: leakage between
    the two, or a pairing error, scales with that pair and not with the clip.  Both sides are compared clipped to [lo, hi]
    (1-Lipschitz); where the reference clips to hi, m_gpu >= hi - delta is asserted in that stricter form.  Entries t >= Tb
    must be zero.  Returns (ref, worst error / bound)."""
    k, min_db, ref_db, max_abs = (float(np.float32(v)) for v in (k, min_db, ref_db, max_abs))       # what the kernel is handed
    if ref is None:
        ref = mel64(x, length, basis, bands, n_fft, hop, k, min_db, ref_db, max_abs)
    out_gpu = np.asarray(out_gpu, dtype=np.float64)
    assert out_gpu.shape == ref.out.shape, (tag, out_gpu.shape, ref.out.shape)
    assert np.isfinite(out_gpu).all() and out_gpu.min() >= 0.0 and out_gpu.max() <= float(np.float32(max_abs)), tag
    delta = REL * pair_peak(ref.X)[None, :] * ref.rows[:, None]
    m_gpu, lo, hi = amplitude_of(out_gpu[:, :ref.Tb], min_db, ref_db, max_abs)
    m_clip = np.clip(ref.m, lo, hi)
    bound = delta + REL * m_clip
    err = np.abs(m_gpu - m_clip)
    worst = float((err / bound).max())
    at_lo, at_hi = ref.m <= lo, ref.m >= hi
    if not quiet:
        print(f"[{tag}] worst |m - m_ref| / bound = {worst:.3e}; max |d out| = {np.abs(out_gpu - ref.out).max():.3e}; "
              f"clipped low {int(at_lo.sum())}, high {int(at_hi.sum())} of {ref.m.size}")
    assert (err <= bound).all(), (tag, worst)
    assert (m_gpu[at_hi] >= hi - delta[at_hi]).all(), tag
    assert not out_gpu[:, ref.Tb:].any(), (tag, "frames past the clip's end")
    return ref, worst


def mel32_paired(x, length, basis, bands, n_fft, hop, k, min_db, ref_db, max_abs):
    """The kernel's method restated in fp32 on the CPU, for calibrating check_mel's bound without the kernel: frames 2q and 2q+1 as
    the real and imaginary part of ONE complex64 torch.fft.fft, separated by Hermitian symmetry, moduli, band product, dB,
    normalise, clip, every step in float32.  Returns out (n_mels, T) float32."""
    import torch
    f32 = np.float32
    L = len(x)
    y = np.asarray(x, dtype=f32)[:length]
    p = y.copy()
    p[1:] = y[1:] - f32(k) * y[:-1]
    T, Tb = 1 + L // hop, 1 + length // hop
    fr = (frames_of(p, n_fft, hop, Tb) * hann_periodic(n_fft).astype(f32)[None, :]).astype(f32)
    if Tb % 2:
        fr = np.concatenate([fr, np.zeros((1, n_fft), f32)])
    z = torch.complex(torch.from_numpy(fr[0::2].copy()), torch.from_numpy(fr[1::2].copy()))
    Z = torch.fft.fft(z, dim=1)
    C = torch.conj(Z[:, (-torch.arange(n_fft)) % n_fft])
    F = n_fft // 2 + 1
    X0 = (0.5 * (Z + C)).abs()[:, :F].numpy().astype(f32)
    X1 = (0.5 * (Z - C)).abs()[:, :F].numpy().astype(f32)
    mag = np.stack([X0, X1], axis=1).reshape(-1, F)[:Tb]                          # (Tb, F)
    m = (band_matrix(basis, bands).astype(f32) @ mag.T).astype(f32)
    S = (f32(20.0) * np.log10(np.maximum(f32(floor_amp(min_db)), m)).astype(f32) - f32(ref_db)).astype(f32)
    v = np.clip(f32(max_abs) * ((S - f32(min_db)) / f32(-min_db)), f32(0), f32(max_abs)).astype(f32)
    out = np.zeros((m.shape[0], T), f32)
    out[:, :Tb] = v
    return out


def floor_value(min_db, ref_db, max_abs):
    """(the normalised value of an empty row in fp64, the tolerance it is held to).  The level 20 log10(floor) - ref_db and the
    difference S - min_db are formed at magnitudes up to D = max(|min_db|, |min_db - ref_db|) dB; log10f (its result scaled by 20)
    and those subtractions round there, and the slope max_abs / (-min_db) carries the error to the output: 4 ulp of D through that
    slope.  (An ulp of the RESULT would not do: where the level cancels against min_db the result is small or zero, -80 + 80 in
    the second parameter set, while the roundings happened at 80.)"""
    min_db, ref_db, max_abs = (float(np.float32(v)) for v in (min_db, ref_db, max_abs))
    want = float(normalise(np.zeros(1), min_db, ref_db, max_abs, floor=floor_amp(min_db))[0])
    D = max(abs(min_db), abs(min_db - ref_db))
    return want, 4.0 * float(np.spacing(np.float32(D))) * max_abs / (-min_db)


# ---- bases ---------------------------------------------------------------------------------------------------------------------
OUTSIDE = np.float32(1e30)              # what `basis` holds outside each row's run: the contract is that it is not read there
SINGLE_W = 0.02                         # weight of a single-bin row: 0.1 (-1)^n with k = 0.97 puts 202 on Nyquist at n_fft 2048
FULL_ROWS = ("bin0", "bin1", "binN/2-1", "binN/2", "full", "hot", "empty")


def _finish(rows, F):
    basis = np.full((len(rows), F), OUTSIDE, dtype=np.float32)
    bands = np.empty((len(rows), 2), dtype=np.int32)
    for j, (f0, f1, w) in enumerate(rows):
        bands[j] = (f0, f1)
        if f0 <= f1:
            basis[j, f0:f1 + 1] = w
    for a in (basis, bands):
        a.setflags(write=False)
    return basis, bands


def full_basis(n_fft, extra=5, single_w=SINGLE_W):
    """(basis (n_mels, F) float32, bands (n_mels, 2) int32, names): single-bin rows at 0, 1, N/2-1 and N/2, a row over the whole
    spectrum with small weights, a 'hot' row over the whole spectrum whose weights push loud frames past the upper clip, one empty
    row (first > last), and `extra` random non-negative rows over random runs."""
    F = n_fft // 2 + 1
    rs = np.random.RandomState(n_fft)
    rows = [(0, 0, single_w), (1, 1, single_w), (F - 2, F - 2, single_w), (F - 1, F - 1, single_w),
            (0, F - 1, rs.uniform(0.0, 2.5e-4, F)), (0, F - 1, rs.uniform(0.0, 0.1, F)), (7, 6, None)]
    for _ in range(extra):
        f0 = int(rs.randint(0, F - 1))
        f1 = int(rs.randint(f0, min(F, f0 + 40)))
        rows.append((f0, f1, rs.uniform(0.0, 0.02, f1 - f0 + 1)))
    return _finish(rows, F) + (FULL_ROWS + tuple(f"run{i}" for i in range(extra)),)


def runs_basis(n_fft, n_mels):
    """n_mels random non-negative rows over random runs (row 0 reaches bin 0, the last row Nyquist; row 1, if any, is empty when
    n_mels > 2)."""
    F = n_fft // 2 + 1
    rs = np.random.RandomState(7 * n_fft + n_mels)
    rows = []
    for j in range(n_mels):
        f0 = 0 if j == 0 else int(rs.randint(0, F - 1))
        f1 = F - 1 if j == n_mels - 1 else int(rs.randint(f0, min(F, f0 + 30)))
        rows.append((f0, f1, rs.uniform(0.0, 0.02, f1 - f0 + 1)))
    if n_mels > 2:
        rows[1] = (3, 2, None)
    return _finish(rows, F) + (tuple(f"run{j}" for j in range(n_mels)),)


def basis_of(case):
    return full_basis(case.n_fft, single_w=case.single_w) if case.basis == "full" else runs_basis(case.n_fft, case.basis)


# ---- signals -------------------------------------------------------------------------------------------------------------------
def signal(kind, n, n_fft, seed):
    """float32 clip of n samples."""
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    if kind == "noise":
        y = rs.randn(n)
        y = y / np.abs(y).max() * 0.9
    elif kind == "dc":
        y = np.full(n, 0.1)
    elif kind == "nyquist":
        y = 0.1 * (-1.0) ** i
    elif kind == "sine":                                    # an exact bin centre
        y = 0.9 * np.sin(2 * np.pi * (n_fft // 8 + 1) * i / n_fft)
    elif kind == "graded":                                  # noise from 1e-4 to 0.9: both ends of the dB range are reached
        y = rs.randn(n)
        y = y / np.abs(y).max() * 0.9 * 10.0 ** (-4.0 * (1.0 - i / max(1, n - 1)))
    elif kind in ("loud_odd", "loud_even"):                 # hop = n_fft: frame t is samples [t N - N/2, t N + N/2)
        y = rs.randn(n)
        y = y / np.abs(y).max() * 0.9
        t = (i + n_fft // 2) // n_fft
        y[(t % 2 == 0) if kind == "loud_odd" else (t % 2 == 1)] = 0.0
    else:
        raise ValueError(kind)
    return y.astype(np.float32)


def mel_case(family, n_fft, hop, L, lens, kinds, basis="full", params=DEFAULT_PARAMS, single_w=SINGLE_W, note=""):
    c = types.SimpleNamespace(family=family, n_fft=n_fft, hop=hop, L=L, lens=list(lens), kinds=list(kinds), basis=basis, params=params,
                              single_w=single_w, B=len(lens), T=1 + L // hop)
    c.tag = f"{family}-N{n_fft}-h{hop}-L{L}-B{c.B}" + (f"-{note}" if note else "")
    assert len(c.kinds) == c.B and all(n_fft // 2 < n <= L for n in c.lens), c.tag
    return c


def mel_wav(case):
    """(B, L) float32, zero-padded rows."""
    wav = np.zeros((case.B, case.L), dtype=np.float32)
    for b, (n, kind) in enumerate(zip(case.lens, case.kinds)):
        wav[b, :n] = signal(kind, n, case.n_fft, 1000 * case.n_fft + 10 * case.hop + b)
    return wav


def hops_of(n_fft):
    return (1, 100, n_fft // 8, n_fft // 4, n_fft // 2 + 1, n_fft, n_fft + 37)


def spectrum_cases():
    out = []
    for N in MEL_NFFTS:
        hop = N // 4
        L = hop * 9 + 5
        out.append(mel_case("spectrum", N, hop, L, [L, L, L - 1, L - hop], ["noise", "dc", "nyquist", "sine"]))
    return out


def hop_cases():
    out = []
    for N in MEL_NFFTS:
        for hop in hops_of(N):
            n = N // 2 + 1 if hop == 1 else N // 2 + 1 + 5 * hop + hop // 3
            out.append(mel_case("hop", N, hop, n, [n], ["noise"]))
    return out


def length_cases():
    return [mel_case("length", N, N // 4, n, [n], ["noise"]) for N in MEL_NFFTS for n in (N // 2 + 1, N // 2 + 2)]


def parity_cases():
    """Batches in which (T parity, T_b parity, T_b < T) takes all six of its combinations (T_b = T has T's parity)."""
    N, hop = 512, 128
    a = mel_case("parity", N, hop, hop * 9 + 5, [hop * 9 + 5, hop * 7 + 1, hop * 6 + 3, N // 2 + 1], ["noise"] * 4, note="Teven")
    b = mel_case("parity", N, hop, hop * 10 + 5, [hop * 10 + 5, hop * 7, hop * 6 + 3, hop * 10], ["noise"] * 4, note="Todd")
    return [a, b]


def parity_combinations(cases):
    return {(c.T % 2, (1 + n // c.hop) % 2, 1 + n // c.hop < c.T) for c in cases for n in c.lens}


def row_cases():
    return [mel_case("rows", 512, 128, 128 * 4 + 3, [128 * 4 + 3, 300], ["noise", "sine"], basis=n, note=f"M{n}") for n in (1, 2, MEL_MAX_ROWS - 1, MEL_MAX_ROWS)]


def param_cases():
    N, hop = 1024, 256
    L = hop * 15 + 9
    return [mel_case("params", N, hop, L, [L, L - 300], ["graded", "noise"], params=p, note=f"p{i}") for i, p in enumerate(PARAM_SETS)]


def leak_cases():
    """hop = n_fft and k = 0: the frames are disjoint, every second one exact zeros.  (8 frames; the clip ends one sample short of
    the last frame's end, so the reflection there stays inside that frame; frame 0's reflection reaches sample N/2 of frame 1 only
    under the window's exact zero.)"""
    return [mel_case("leak", N, N, 7 * N + N // 2 - 1, [7 * N + N // 2 - 1], [kind], params=LEAK_PARAMS, single_w=0.05, note=kind) for N in MEL_NFFTS for kind in ("loud_odd", "loud_even")]


def mel_cases():
    return spectrum_cases() + hop_cases() + length_cases() + parity_cases() + row_cases() + param_cases() + leak_cases()


# ==================================================================================================================================
# pre-emphasis
# ==================================================================================================================================
PRE_KS = (0.0, 0.97, -0.5, 1.0)
PRE_SHAPES = [(5, L) for L in (1, 2, EW_THREADS - 1, EW_THREADS, EW_THREADS + 1)] + [(3, EW_BLOCKS * EW_THREADS // 3 + 1)]


def preemphasis64(x, k):
    """x (B, L) float32 -> (p float64, bound): p[n] = x[n] - k x[n-1], p[0] = x[0] per row, k at its fp32 value; bound =
    2 * 2^-24 (|x[n]| + |k x[n-1]|): the product and the difference each round once (one rounding under contraction)."""
    k = float(np.float32(k))
    x = np.asarray(x, dtype=np.float64)
    p, mag = x.copy(), np.abs(x)
    p[:, 1:] -= k * x[:, :-1]
    mag[:, 1:] += np.abs(k * x[:, :-1])
    return p, 2.0 * U32 * mag


# ==================================================================================================================================
# resampler
# ==================================================================================================================================
def resample_sum(x, length, table, P, Q, W, dtype=np.int64):
    """out[m] = sum_j x[floor(m Q / P) - W + 1 + j] * table[j][m mod P], j = 0 .. 2W - 1, for m < ceil(length P / Q), zero up to
    L_out = ceil(L_in P / Q); x zero outside [0, length).  table (2W, P) in the kernel's layout.  Returns (out, sum of |terms|)."""
    x = np.asarray(x)
    L_out = cdiv(len(x) * P, Q)
    n_out = cdiv(length * P, Q)
    out, mag = np.zeros(L_out, dtype=dtype), np.zeros(L_out, dtype=dtype)
    table = np.asarray(table).astype(dtype)
    xs = x.astype(dtype)
    for m0 in range(0, n_out, 4096):                        # in slabs, to bound the gather's memory
        m = np.arange(m0, min(n_out, m0 + 4096), dtype=np.int64)
        n = (m * Q // P - W + 1)[:, None] + np.arange(2 * W, dtype=np.int64)[None, :]
        xn = np.where((n >= 0) & (n < length), xs[np.clip(n, 0, max(0, len(x) - 1))], 0)
        c = table[:, m % P].T
        out[m] = (xn * c).sum(axis=1)
        mag[m] = (np.abs(xn) * np.abs(c)).sum(axis=1)
    return out, mag


# (P, Q, W): P = 1, Q = 1, P > Q and P < Q with the smallest half widths and the production one, the two production ratios with a
# table wider / narrower than a tile, and the widest span the launcher accepts
RS_PROBES = [(1, 3, 5), (3, 1, 4)] + [(3, 2, W) for W in (1, 2, 3, 64)] + [(2, 3, W) for W in (1, 2, 3, 64)] + [
    (441, 320, 64), (147, 640, 279), (1, 42, 2688)]
RS_REFUSED_LDS = (1, 43, 2752)          # ceil(64 * 43): 65880 bytes
RS_TILES = 5                            # tiles of the probes' row
RS_ROUNDING = [(22050, 8000, 3001), (96000, 22050, 5001), (42, 1, 12000)]      # (sr_in, sr_out, samples)


def rs_row(P, Q):
    """L_in of the probes' row: RS_TILES tiles, the last one partial."""
    return ((RS_TILES - 1) * RS_TILE + 77) * Q // P


def rs_boundary(P, Q, kth):
    """The input length a whose output ends at the kth tile boundary or just before it: ceil(a P / Q) <= kth 256 <
    ceil((a + 1) P / Q)."""
    return kth * RS_TILE * Q // P


def rs_lengths(P, Q):
    """0 and 1, either side of the first, second and last tile boundary, a clip whose last tiles lie wholly past its end, the row."""
    L_in = rs_row(P, Q)
    tiles = cdiv(cdiv(L_in * P, Q), RS_TILE)
    lens = [0, 1]
    for kth in (1, 2, tiles - 1):
        a = rs_boundary(P, Q, kth)
        lens += [a, a + 1]
    return lens + [rs_boundary(P, Q, 1) + rs_boundary(P, Q, 1) // 2, L_in]


def rs_probe(P, Q, W):
    """(wav (B, L_in) integers in [-8, 8] as float32, zero-padded; lens; table (2W, P) integers in [-8, 8] as float32)."""
    rs = np.random.RandomState(P * 1000 + Q * 10 + W)
    lens = rs_lengths(P, Q)
    L_in = rs_row(P, Q)
    order = rs.permutation(len(lens))
    lens = [lens[i] for i in order]
    wav = np.zeros((len(lens), L_in), dtype=np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = rs.randint(-8, 9, n)
    return wav, lens, rs.randint(-8, 9, (2 * W, P)).astype(np.float32)


# ==================================================================================================================================
# trim
# ==================================================================================================================================
TRIM_SHAPES = [(2, 1), (64, 16), (512, 128), (2048, 512), (TRIM_MAX_FRAME, 2048), (1000, 300), (64, 200)]
TOP_DB = 20.0
TRIM_STARTS, TRIM_ENDS = (TRIM_BLOCK - 1, TRIM_BLOCK, TRIM_BLOCK + 1, 600), (2 * TRIM_BLOCK - 1, 2 * TRIM_BLOCK, None)   # None: the last frame


def frame_energy_sums(x, length, N, hop):
    """int64 (Tb,): sum over the frame of p^2, p = reflect_pad(x[0:length], N/2)[t hop : t hop + N], for integer samples."""
    y = np.asarray(x)[:length].astype(np.int64)
    assert (y == np.asarray(x)[:length]).all()
    fr = frames_of(y, N, hop, 1 + length // hop)
    return (fr * fr).sum(axis=1)


def trim_clip(length, N, hop, first, last, seed):
    """Integer samples in [-15, 15] as float32: frames first .. last (last None: the clip's last frame) hold samples of
    magnitude 12 .. 15 wherever no frame outside that range reaches; everything else is +-1 on every 32nd sample (N >= 64) or
    exact zeros (N < 64), at least 30 dB below the loudest frame (the host test asserts it from the integer energies)."""
    rs = np.random.RandomState(seed)
    y = np.zeros(length, dtype=np.int64)
    if N >= 64:
        y[5::32] = rs.choice([-1, 1], len(y[5::32]))
    Tb = 1 + length // hop
    a = max(0, (first - 1) * hop + N // 2) if first > 0 else 0
    b = length if last is None or last >= Tb - 1 else (last + 1) * hop - N // 2
    assert 0 <= a < b <= length, (length, N, hop, first, last)
    y[a:b] = rs.randint(12, 16, b - a) * rs.choice([-1, 1], b - a)
    return y.astype(np.float32)


def trim_block_batch():
    """(N, hop, clips): 900 to 1100 frames at (64, 16): trim_bounds_kernel's loops run four or five passes, and the loud region
    starts and ends on the last frame of a pass, the first of the next and one further, so both tree reductions meet threads
    that hold more than one live value."""
    N, hop = 64, 16
    clips, want = [], []
    combos = [(s, e) for s in TRIM_STARTS[:3] for e in TRIM_ENDS] + [(TRIM_STARTS[3], None)]
    for i, (s, e) in enumerate(combos):
        Tb = 900 + (i * 23) % 201
        length = (Tb - 1) * hop + (i * 5) % hop
        clips.append(trim_clip(length, N, hop, s, e, seed=i))
        want.append((s, Tb - 1 if e is None else e))
    return N, hop, clips, want


def trim_shape_batch(N, hop):
    """A clip with a loud middle, the shortest legal clip (len = N/2 + 1: one frame when hop > len) and an all-zero clip."""
    short = N // 2 + 1
    mid = max(short, 20 * hop + 7)
    clips = [trim_clip(mid, N, hop, 6, 13, seed=N + hop), trim_clip(short, N, hop, 0, None, seed=N), np.zeros(mid - 1, dtype=np.float32)]
    return clips


# ==================================================================================================================================
# exact comparison
# ==================================================================================================================================
def assert_same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert not len(bad), (tag, f"{len(bad)} of {got.size} differ, first at {int(bad[0])}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")
