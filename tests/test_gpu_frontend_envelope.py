"""The wav -> mel front end's kernels across their envelope (csrc/audio.hip: melspectrogram_kernel, preemphasis_kernel;
csrc/resample.hip: resample_kernel, frame_energy_kernel, trim_bounds_kernel), called through the raw entry points with the
caller's own basis, bands, table and parameters, against tests/helpers/frontend_ref64.py (whose tables, exactness conditions and
comparison rules tests/test_frontend_ref_host.py checks on the CPU).

Every input and every output is a view into a larger buffer: NaN (int32 outputs: a sentinel) on either side, checked after each
call, and an output is NaN-filled before the call, so an element that is not written shows.  `basis` holds 1e30 outside each
row's [first, last]: the contract is that it is not read there.  Every test prints its figures before it asserts; the module
prints its worst error / bound per family and its wall time when it ends (pytest -s)."""
import time
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio as Au
from neural_sound_generation_amd.ops import _p, _stream
from tests.helpers import frontend_ref64 as R, resample64 as R64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

GUARD = 1024                    # elements of NaN / sentinel on either side of every buffer
SENTINEL = -7777
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print(f"\n[frontend envelope] worst error / bound per family: { {k: f'{v:.3e}' for k, v in WORST.items()} }; "
          f"wall time {time.time() - t0:.1f} s")


def note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), float(worst))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def guarded(shape, dtype=torch.float32, host=None):
    """(buffer, view of `shape` inside it): the view holds `host` or, for an output, NaN / the sentinel like its surroundings."""
    n = int(np.prod(shape))
    fill = float("nan") if dtype == torch.float32 else SENTINEL
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if host is not None:
        view.copy_(torch.from_numpy(np.array(host)).view(*shape))
    return buf, view


def untouched(buf, lo=GUARD, hi=None):
    """The guards of a buffer (or, lo = hi = 0 .. all of it) still hold what they were filled with."""
    whole = buf.cpu().numpy()
    hi = len(whole) - GUARD if hi is None else hi
    edge = np.concatenate([whole[:lo], whole[hi:]])
    return bool(np.isnan(edge).all()) if whole.dtype == np.float32 else bool((edge == SENTINEL).all())


def status(name, *args):
    """(status, message) of a raw call: no exception."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.nsg_last_error_string()
    return rc, (msg.decode() if msg else "")


# ==================================================================================================================================
# melspectrogram
# ==================================================================================================================================
def run_mel(wav, lens, basis, bands, n_fft, hop, params, frame_major=0):
    """(B, n_mels, T) float32 numpy (a frame-major result is transposed on the host); lens None: lengths = NULL."""
    B, L = wav.shape
    n_mels, T = basis.shape[0], 1 + L // hop
    assert basis.shape[1] == n_fft // 2 + 1 and bands.shape == (n_mels, 2) and bands.dtype == np.int32
    wbuf, wd = guarded((B, L), host=wav)
    bbuf, bd = guarded(basis.shape, host=basis)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    obuf, out = guarded((B, T, n_mels) if frame_major else (B, n_mels, T))
    bands = np.ascontiguousarray(bands)
    _lib.call("nsg_audio_melspectrogram", _p(wd), _p(ld), _p(bd), c_void_p(bands.ctypes.data), _p(out), B, L, n_fft, hop, n_mels,
              *params, frame_major, _stream())
    torch.cuda.synchronize()
    assert untouched(obuf) and untouched(wbuf) and untouched(bbuf), "a store outside the output"
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), "an output element was not written (or NaN was read from outside an input)"
    return got.transpose(0, 2, 1) if frame_major else got


def run_case(c, frame_major=0):
    basis, bands, names = R.basis_of(c)
    wav = R.mel_wav(c)
    lens = None if all(n == c.L for n in c.lens) else c.lens
    return basis, bands, names, wav, run_mel(wav, lens, basis, bands, c.n_fft, c.hop, c.params, frame_major)


def check_case(c, basis, bands, names, wav, got):
    worst = 0.0
    for b in range(c.B):
        ref, w = R.check_mel(got[b], wav[b], c.lens[b], basis, bands, c.n_fft, c.hop, *c.params, tag=f"{c.tag}/{b}:{c.kinds[b]}")
        assert (bits(got[b][:, ref.Tb:]) == 0).all(), "frames past the clip's end are +0.0"
        worst = max(worst, w)
        for j, n in enumerate(names):
            if bands[j, 0] > bands[j, 1]:                                     # an empty row: the floor's value in every frame
                want, tol = R.floor_value(*c.params[1:])
                d = np.abs(got[b][j, :ref.Tb].astype(np.float64) - want).max()
                print(f"[{c.tag}/{b}] empty row {n}: floor value {want:.9g}, max |d| = {d:.3e} (tolerance {tol:.3e}, ulp of the value {np.spacing(np.float32(want)):.3e})")
                assert d <= tol
    note("mel " + c.family, worst)
    return worst


@pytest.mark.parametrize("c", R.spectrum_cases(), ids=lambda c: c.tag)
def test_mel_full_spectrum_bases(c):
    """Single-bin rows at DC, 1, N/2-1 and Nyquist, a row over the whole spectrum, random runs and an empty row, on white noise, a
    constant, (-1)^n and a sine at an exact bin centre."""
    check_case(c, *run_case(c))


@pytest.mark.parametrize("c", R.hop_cases() + R.length_cases() + R.parity_cases(), ids=lambda c: c.tag)
def test_mel_hops_lengths_and_parities(c):
    check_case(c, *run_case(c))


@pytest.mark.parametrize("n_fft", R.MEL_NFFTS)
def test_mel_clip_does_not_depend_on_its_batch(n_fft):
    """The same clip at b = 0 of B = 1 with L = len (T odd), and at b = 6 of B = 7 in a wider row (T even): bit for bit."""
    hop = n_fft // 4
    n, L = hop * 6 + 17, hop * 9 + 5
    basis, bands, _ = R.full_basis(n_fft)
    clip = R.signal("noise", n, n_fft, 5)
    alone = run_mel(clip[None], None, basis, bands, n_fft, hop, R.DEFAULT_PARAMS)
    lens = [L, n_fft // 2 + 1, hop * 4, L - 1, hop * 7 + 3, n + 1, n]
    wav = np.zeros((7, L), dtype=np.float32)
    for b, m in enumerate(lens[:-1]):
        wav[b, :m] = R.signal("noise", m, n_fft, 50 + b)
    wav[6, :n] = clip
    batch = run_mel(wav, lens, basis, bands, n_fft, hop, R.DEFAULT_PARAMS)
    Tb = 1 + n // hop
    assert alone.shape[2] == Tb == 7 and batch.shape[2] == 10
    diff = int((bits(batch[6][:, :Tb]) != bits(alone[0])).sum())
    print(f"[N{n_fft}] alone vs row 6 of 7: {diff} of {alone[0].size} entries differ")
    assert diff == 0 and (bits(batch[6][:, Tb:]) == 0).all()
    R.check_mel(alone[0], clip, n, basis, bands, n_fft, hop, *R.DEFAULT_PARAMS, tag=f"alone-N{n_fft}")


@pytest.mark.parametrize("c", R.row_cases(), ids=lambda c: c.tag)
def test_mel_rows_and_layouts(c):
    """n_mels 1, 2, 127, 128 (the thread map m = tid & 127 and its limit); the two layouts are transposes bit for bit."""
    basis, bands, names, wav, a = run_case(c, 0)
    _, _, _, _, b = run_case(c, 1)
    diff = int((bits(a) != bits(b)).sum())
    print(f"[{c.tag}] mel-major vs frame-major: {diff} of {a.size} entries differ")
    assert a.shape == (c.B, c.basis, c.T) and diff == 0
    check_case(c, basis, bands, names, wav, a)


@pytest.mark.parametrize("c", R.param_cases(), ids=lambda c: c.tag)
def test_mel_parameters(c):
    """Pre-emphasis 0, negative and 1; three dB ranges; max_abs 4 and 0.5; the third set's floor comes out at 0.2."""
    basis, bands, names, wav, got = run_case(c)
    check_case(c, basis, bands, names, wav, got)
    if c.params[2] < 0:
        lo = float(got[:, :, :1 + min(c.lens) // c.hop].min())
        print(f"[{c.tag}] smallest output {lo:.9g}")
        assert abs(lo - 0.2) <= R.floor_value(*c.params[1:])[1]


@pytest.mark.parametrize("c", R.leak_cases(), ids=lambda c: c.tag)
def test_mel_quiet_frame_beside_a_loud_one(c):
    """Disjoint frames, every second one exact zeros: what a quiet frame shows is what its partner in the complex FFT leaked, held
    to the PAIR's delta."""
    basis, bands, names, wav, got = run_case(c)
    ref = R.mel64(wav[0], c.lens[0], basis, bands, c.n_fft, c.hop, *c.params)
    quiet = np.arange(0 if c.kinds[0] == "loud_odd" else 1, ref.Tb, 2)
    m_gpu, lo, hi = R.amplitude_of(got[0], *c.params[1:])
    single = [j for j in range(len(names)) if bands[j, 0] == bands[j, 1]]
    leak = np.where(m_gpu[single][:, quiet] > lo * (1 + 1e-4), m_gpu[single][:, quiet], 0.0) / c.single_w       # |X| of one bin
    frac = leak / R.pair_peak(ref.X)[quiet][None, :]
    print(f"[{c.tag}] largest leaked bin amplitude / partner's peak = {frac.max():.3e} (0: every quiet entry sits on the floor, which shows below "
          f"{lo / c.single_w / R.pair_peak(ref.X)[quiet].min():.1e} of the partner's peak; the bound allows REL = {R.REL:.0e})")
    note("mel leak / partner's peak", frac.max())
    assert not ref.X[:, quiet].any()
    check_case(c, basis, bands, names, wav, got)


# ==================================================================================================================================
# pre-emphasis
# ==================================================================================================================================
@pytest.mark.parametrize("k", R.PRE_KS)
@pytest.mark.parametrize("B,L", R.PRE_SHAPES)
def test_preemphasis(B, L, k):
    x = np.random.RandomState(B * L % 9973).standard_normal((B, L)).astype(np.float32)
    xbuf, xd = guarded((B, L), host=x)
    ybuf, yd = guarded((B, L))
    _lib.call("nsg_audio_preemphasis", _p(xd), _p(yd), B, L, k, _stream())
    torch.cuda.synchronize()
    assert untouched(ybuf) and untouched(xbuf)
    got = yd.cpu().numpy()
    want, bound = R.preemphasis64(x, k)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[preemphasis B{B} L{L} k{k}] max error {err.max():.3e}, max error / bound {ratio:.3e}")
    note("preemphasis", ratio)
    assert not np.isnan(got).any() and (err <= bound).all()
    assert (bits(got[:, 0]) == bits(x[:, 0])).all(), "p[b][0] == x[b][0] exactly"


# ==================================================================================================================================
# resampler
# ==================================================================================================================================
def run_resample(wav, lens, table, P, Q, W):
    B, L_in = wav.shape
    L_out = R.cdiv(L_in * P, Q)
    assert table.shape == (2 * W, P)
    wbuf, wd = guarded((B, L_in), host=wav)
    tbuf, td = guarded(table.shape, host=table)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    obuf, out = guarded((B, L_out))
    _lib.call("nsg_audio_resample", _p(wd), _p(ld), _p(td), _p(out), B, L_in, P, Q, W, _stream())
    torch.cuda.synchronize()
    assert untouched(obuf) and untouched(wbuf) and untouched(tbuf)
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


@pytest.mark.parametrize("P,Q,W", R.RS_PROBES)
def test_resample_exact_probes(P, Q, W):
    """Integer samples and an integer table: the kernel must EQUAL the int64 restatement, on a shuffled ragged batch whose clips
    end at 0 and 1 samples, either side of the first, second and last tile boundary, and tiles short of the row's end; and each
    clip alone is bit for bit its row of the batch."""
    wav, lens, table = R.rs_probe(P, Q, W)
    got = run_resample(wav, lens, table, P, Q, W)
    print(f"[resample probe {P}/{Q} W{W}] {len(lens)} clips of {lens} samples in rows of {wav.shape[1]}; LDS {R.rs_lds_bytes(P, Q, W)} bytes")
    for b, n in enumerate(lens):
        want, _ = R.resample_sum(wav[b], n, table, P, Q, W)
        R.assert_same(got[b], want, tag=f"{P}/{Q} W{W} clip {b} of {n} samples")
        if n:
            alone = run_resample(wav[b:b + 1, :n], None, table, P, Q, W)
            n_out = R.cdiv(n * P, Q)
            assert alone.shape == (1, n_out) and (bits(alone[0]) == bits(got[b, :n_out])).all(), (b, n)
        assert (bits(got[b, R.cdiv(n * P, Q):]) == 0).all()


@pytest.mark.parametrize("sr_in,sr_out,n", R.RS_ROUNDING)
def test_resample_rounding(sr_in, sr_out, n):
    """The real table on noise, at the ratios with the widest filters (W = 177, 279 and 2688: 42 -> 1 fills 64348 of the 65536
    bytes of LDS the launcher allows)."""
    P, Q = R64.ratio(sr_in, sr_out)
    W = R64.half_width(P, Q)
    table = Au._resample_table_on(P, Q, "cpu").numpy()
    x = np.random.RandomState(n).uniform(-1, 1, n).astype(np.float32)
    got = run_resample(x[None], None, table, P, Q, W)[0]
    y64, A = R64.resample64(x, sr_in, sr_out)
    bound = (2 * W + 2) * 2.0 ** -24 * A + 1e-12
    err = np.abs(got.astype(np.float64) - y64)
    print(f"[resample {sr_in} -> {sr_out}, {n} samples, W {W}] max |y - y64| = {err.max():.3e}, max error / bound = {(err / bound).max():.3e}")
    note("resample rounding", (err / bound).max())
    assert got.shape == y64.shape and (err <= bound).all()


# ==================================================================================================================================
# trim
# ==================================================================================================================================
def run_trim(clips, N, hop, pad=37):
    """(bounds (B, 2), energies: per clip the fp32 mse of its frames) of a ragged batch in rows `pad` wider than the longest."""
    lens = [len(y) for y in clips]
    B, L = len(clips), max(lens) + pad
    wav = np.zeros((B, L), dtype=np.float32)
    for b, y in enumerate(clips):
        wav[b, :lens[b]] = y
    T = 1 + L // hop
    nb = _lib.query("nsg_audio_trim_workspace_bytes", B, L, hop)
    assert nb >= B * T * 4 and nb % 4 == 0
    wbuf, wd = guarded((B, L), host=wav)
    sbuf, ws = guarded((nb // 4,))
    bbuf, bd = guarded((B, 2), dtype=torch.int32)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.call("nsg_audio_trim_bounds", _p(wd), _p(ld), _p(bd), B, L, N, hop, R.TOP_DB, _p(ws), nb, _stream())
    torch.cuda.synchronize()
    assert untouched(bbuf) and untouched(sbuf) and untouched(wbuf)
    mse = ws.cpu().numpy()[:B * T].reshape(B, T)                                   # resample.hip frame_energy_kernel: mse[b T + t]
    return bd.cpu().numpy(), [mse[b, :1 + lens[b] // hop] for b in range(B)]


def check_trim(clips, N, hop, tag):
    bounds, energies = run_trim(clips, N, hop)
    for b, y in enumerate(clips):
        sums = R.frame_energy_sums(y, len(y), N, hop)
        assert sums.max() < R.EXACT_SUM
        want_e = sums.astype(np.float32) / np.float32(N)                            # the sum is exact; the quotient rounds once
        ulps = np.abs(energies[b].astype(np.float64) - want_e) / np.spacing(np.maximum(want_e, np.float32(1e-30)))
        (start, end), margin = R64.trim64(y, R.TOP_DB, N, hop)
        print(f"[{tag} clip {b}: {len(y)} samples, {len(sums)} frames] energies off by at most {ulps.max():.1f} ulp; bounds {tuple(bounds[b])}, "
              f"trim64 {(start, end)}, margin {margin:.2f} dB")
        assert not np.isnan(energies[b]).any()
        assert ulps.max() == 0 if N & (N - 1) == 0 else ulps.max() <= 1, "integer samples: a frame's energy sum is exact"
        assert margin >= 0.01
        R.assert_same(bounds[b], np.array((start, end)), tag=f"{tag} clip {b}")
    return bounds


def test_trim_bounds_over_several_passes_of_256_frames():
    """900 to 1100 frames a clip at (64, 16): the loud region starts on frame 255, 256, 257 or 600 and ends on 511, 512 or the last."""
    N, hop, clips, want = R.trim_block_batch()
    check_trim(clips, N, hop, "trim passes")
    bounds, _ = run_trim(clips[::-1], N, hop, pad=5)                                # another order, another row width
    R.assert_same(bounds[::-1], np.array([R64.trim64(y, R.TOP_DB, N, hop)[0] for y in clips]))


@pytest.mark.parametrize("N,hop", R.TRIM_SHAPES)
def test_trim_exact_energies(N, hop):
    """Every frame length's edge (2, 8192, one that is no power of two), hop > frame_length, the shortest legal clip and an
    all-zero clip, which keeps all of itself."""
    clips = R.trim_shape_batch(N, hop)
    bounds = check_trim(clips, N, hop, f"trim {N}/{hop}")
    assert tuple(bounds[2]) == (0, len(clips[2])) and tuple(bounds[1]) == (0, N // 2 + 1)


# ==================================================================================================================================
# refusals
# ==================================================================================================================================
def refused(name, args, want_status, pattern, outputs):
    import re
    rc, msg = status(name, *args)
    torch.cuda.synchronize()
    print(f"[{name}] status {rc}: {msg}")
    assert rc == want_status and msg.startswith(name) and re.search(pattern, msg), (rc, msg)
    for buf in outputs:
        assert untouched(buf, 0, 0), "a refused call wrote to its output"


MEL_OK = dict(B=2, L=600, n_fft=512, hop=128, n_mels=4, k=0.97, min_db=-100.0, ref_db=20.0, max_abs=1.0, frame_major=0)
MEL_REFUSALS = [
    ("wav", dict(wav=None), R.E_INVALID, "bad argument"), ("basis", dict(basis=None), R.E_INVALID, "bad argument"),
    ("bands", dict(bands=None), R.E_INVALID, "bad argument"), ("out", dict(out=None), R.E_INVALID, "bad argument"),
    ("B0", dict(B=0), R.E_INVALID, "bad argument"), ("L0", dict(L=0), R.E_INVALID, "bad argument"),
    ("hop0", dict(hop=0), R.E_INVALID, "bad argument"), ("hop-1", dict(hop=-1), R.E_INVALID, "bad argument"),
    ("n_mels0", dict(n_mels=0), R.E_INVALID, "bad argument"),
    ("max_abs0", dict(max_abs=0.0), R.E_INVALID, "max_abs_value > 0"), ("min_db0", dict(min_db=0.0), R.E_INVALID, "min_level_db < 0"),
    ("frame_major2", dict(frame_major=2), R.E_INVALID, "frame_major 0 or 1"), ("frame_major-1", dict(frame_major=-1), R.E_INVALID, "frame_major 0 or 1"),
    ("n_fft256", dict(n_fft=256), R.E_UNSUPPORTED, "n_fft must be 512, 1024 or 2048"), ("n_fft1000", dict(n_fft=1000), R.E_UNSUPPORTED, "n_fft must be"),
    ("n_fft4096", dict(n_fft=4096, L=2100), R.E_UNSUPPORTED, "n_fft must be"),
    ("n_mels129", dict(n_mels=R.MEL_MAX_ROWS + 1), R.E_UNSUPPORTED, "at most 128 mel bins"),
    ("L=n_fft/2", dict(L=256), R.E_UNSUPPORTED, "more than n_fft/2 samples"),
    ("band-1", dict(band=(2, 0, -1)), R.E_INVALID, "band index outside"), ("bandF", dict(band=(1, 1, 257)), R.E_INVALID, "band index outside"),
]


@pytest.mark.parametrize("what,change,want,pattern", MEL_REFUSALS, ids=[r[0] for r in MEL_REFUSALS])
def test_melspectrogram_refusals(what, change, want, pattern):
    """Buffers sized for the largest values any of these cases names (129 rows, n_fft 4096, L 2100), whatever is refused."""
    a = dict(MEL_OK, **{k: v for k, v in change.items() if k in MEL_OK})
    rows, F, Lmax = R.MEL_MAX_ROWS + 1, 4096 // 2 + 1, 2100
    _, wav = guarded((2, Lmax), host=np.zeros((2, Lmax), np.float32))
    _, basis = guarded((rows, F), host=np.full((rows, F), 0.01, np.float32))
    obuf, out = guarded((2, rows, 1 + Lmax))
    bands = np.zeros((rows, 2), dtype=np.int32)
    bands[:, 1] = 5
    if "band" in change:
        r, c, v = change["band"]
        bands[r, c] = v
    ptr = {"wav": _p(wav), "basis": _p(basis), "bands": c_void_p(bands.ctypes.data), "out": _p(out)}
    ptr.update({k: c_void_p(0) for k in change if k in ptr})
    refused("nsg_audio_melspectrogram", (ptr["wav"], c_void_p(0), ptr["basis"], ptr["bands"], ptr["out"], a["B"], a["L"], a["n_fft"], a["hop"], a["n_mels"],
                                         a["k"], a["min_db"], a["ref_db"], a["max_abs"], a["frame_major"], _stream()), want, pattern, [obuf])


def test_preemphasis_refusals():
    xbuf, x = guarded((2, 100), host=np.ones((2, 100), np.float32))
    ybuf, y = guarded((2, 100))
    for args in ((c_void_p(0), _p(y), 2, 100), (_p(x), c_void_p(0), 2, 100), (_p(y), _p(y), 2, 100), (_p(x), _p(y), 0, 100), (_p(x), _p(y), 2, 0),
                 (_p(x), _p(y), -1, 100)):
        refused("nsg_audio_preemphasis", args + (0.97, _stream()), R.E_INVALID, "bad argument", [ybuf])


RS_REFUSALS = [
    ("wav", dict(wav=None), R.E_INVALID, "bad argument"), ("table", dict(table=None), R.E_INVALID, "bad argument"), ("out", dict(out=None), R.E_INVALID, "bad argument"),
    ("B0", dict(B=0), R.E_INVALID, "bad argument"), ("L0", dict(L_in=0), R.E_INVALID, "bad argument"), ("up0", dict(P=0), R.E_INVALID, "bad argument"),
    ("down0", dict(Q=0), R.E_INVALID, "bad argument"), ("W0", dict(W=0), R.E_INVALID, "bad argument"),
    ("6/4", dict(P=6, Q=4), R.E_INVALID, r"up / down = 6 / 4 is not in lowest terms"),
    ("table>2^20", dict(P=4099, Q=1, W=128), R.E_UNSUPPORTED, r"table of ratio 4099 / 1 has 1049344 floats, more than 2\^20"),
    ("1/43", dict(P=R.RS_REFUSED_LDS[0], Q=R.RS_REFUSED_LDS[1], W=R.RS_REFUSED_LDS[2]), R.E_UNSUPPORTED, r"ratio 1 / 43 needs 65880 bytes of LDS"),
]


@pytest.mark.parametrize("what,change,want,pattern", RS_REFUSALS, ids=[r[0] for r in RS_REFUSALS])
def test_resample_refusals(what, change, want, pattern):
    """Every buffer has the size its case's own arguments ask for."""
    a = dict(B=1, L_in=300, P=3, Q=2, W=2)
    a.update({k: v for k, v in change.items() if k in a})
    assert what != "table>2^20" or a["P"] * 2 * a["W"] == R.RS_MAX_TABLE + 768
    P, Q, W = max(1, a["P"]), max(1, a["Q"]), max(1, a["W"])
    _, wav = guarded((1, 300), host=np.ones((1, 300), np.float32))
    _, table = guarded((2 * W, P), host=np.ones((2 * W, P), np.float32))
    obuf, out = guarded((1, R.cdiv(300 * P, Q)))
    ptr = {"wav": _p(wav), "table": _p(table), "out": _p(out)}
    ptr.update({k: c_void_p(0) for k in change if k in ptr})
    refused("nsg_audio_resample", (ptr["wav"], c_void_p(0), ptr["table"], ptr["out"], a["B"], a["L_in"], a["P"], a["Q"], a["W"], _stream()), want, pattern, [obuf])


TRIM_REFUSALS = [
    ("wav", dict(wav=None), R.E_INVALID, "bad argument"), ("bounds", dict(bounds=None), R.E_INVALID, "bad argument"),
    ("B0", dict(B=0), R.E_INVALID, "bad argument"), ("L0", dict(L=0), R.E_INVALID, "bad argument"), ("hop0", dict(hop=0), R.E_INVALID, "hop > 0"),
    ("top_db0", dict(top_db=0.0), R.E_INVALID, "top_db > 0"), ("top_db-1", dict(top_db=-1.0), R.E_INVALID, "top_db > 0"),
    ("N63", dict(N=63), R.E_UNSUPPORTED, r"frame_length must be even and in \[2, 8192\]"), ("N0", dict(N=0), R.E_UNSUPPORTED, "frame_length must be even"),
    ("N8193", dict(N=R.TRIM_MAX_FRAME + 1), R.E_UNSUPPORTED, "frame_length must be even"), ("N8194", dict(N=R.TRIM_MAX_FRAME + 2), R.E_UNSUPPORTED, "frame_length must be even"),
    ("L=N/2", dict(N=1400), R.E_UNSUPPORTED, "more than frame_length/2 samples"),
    ("ws null", dict(ws=None), R.E_WORKSPACE, "workspace too small"), ("ws one byte short", dict(short=1), R.E_WORKSPACE, "workspace too small"),
]


@pytest.mark.parametrize("what,change,want,pattern", TRIM_REFUSALS, ids=[r[0] for r in TRIM_REFUSALS])
def test_trim_refusals(what, change, want, pattern):
    a = dict(B=2, L=700, N=64, hop=16, top_db=20.0)
    a.update({k: v for k, v in change.items() if k in a})
    _, wav = guarded((2, 700), host=np.ones((2, 700), np.float32))
    nb = _lib.query("nsg_audio_trim_workspace_bytes", 2, 700, 16)
    assert nb >= 2 * (1 + 700 // 16) * 4
    sbuf, ws = guarded((nb // 4,))
    bbuf, bounds = guarded((2, 2), dtype=torch.int32)
    ptr = {"wav": _p(wav), "bounds": _p(bounds), "ws": _p(ws)}
    ptr.update({k: c_void_p(0) for k in change if k in ptr})
    refused("nsg_audio_trim_bounds", (ptr["wav"], c_void_p(0), ptr["bounds"], a["B"], a["L"], a["N"], a["hop"], a["top_db"], ptr["ws"],
                                      nb - change.get("short", 0), _stream()), want, pattern, [bbuf, sbuf])


def test_the_refusal_baselines_are_accepted():
    """The arguments the refusal tables start from are legal: each call returns 0 and writes its output."""
    basis, bands, _ = R.runs_basis(512, 4)
    got = run_mel(np.zeros((2, 600), np.float32), None, basis, bands, 512, 128, R.DEFAULT_PARAMS)
    assert got.shape == (2, 4, 5) and not got.any()
    assert run_resample(np.ones((1, 300), np.float32), None, np.ones((4, 3), np.float32), 3, 2, 2).shape == (1, 450)
    bounds, _ = run_trim([np.ones(700, np.float32)] * 2, 64, 16, pad=0)
    assert bounds.tolist() == [[0, 700]] * 2
