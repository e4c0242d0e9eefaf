"""resample_kernel, frame_energy_kernel and trim_bounds_kernel (csrc/resample.hip) across their envelope, called at the C entry
points nsg_audio_resample and nsg_audio_trim_bounds so that the test chooses the table, (up, down, half_width), every buffer and
the workspace.  References and case tables: tests/helpers/resample_envelope.py (tests/test_resample_envelope_host.py checks on the
CPU what they assume).  The boundaries, and the line of resample.hip each belongs to:

    resample_kernel      `table + (int)(m % P)`, `c[j * P]`         integer tables, P = 1 .. 257 (more phases than a tile has outputs)
                         `m * Q / P - W + 1 - lo`                   exact probe at P / Q = 3/2, 2/3, 7/5, 1/1, 257/256, 64/1, 1/64
                         `for (i = tid; i <= hi - lo; ...)`         spans of 1 + 2W floats (64/1) up to 16383 (1/64, W = 31: the LDS limit)
                         `m_last = ... L_out - 1`                   every L_out has a tail tile; L_out = 1, 256, 257 in the runs alone
                         `if (m0 >= len_out)`: zeros                a whole tile past a clip; len = 0; a device length of -5
                         `nsg_clip_at(x, lo + i, len)`              NaN past every clip's length and 67 NaN on either side of wav
    frame_energy_kernel  `for (i = lane; i < N; i += 64)`           N = 2, 62, 64, 66 (idle lanes, one lap, a second lap), 2048, 8192
                         `nsg_reflect_once(start + i, len)`         clips of N/2 + 1 samples (both folds at their longest), loud ends
                         `t >= 1 + len / hop`                       lengths on a multiple of hop and one past it; hop = 1, 7, N/4, 2N
    trim_bounds_kernel   `for (t = tid; t < Tb; t += 256)`          1, 63, 64, 65, 255, 256, 257 and 513 frames
                         `nsg_wave_min(first)`, `wlo[wave]`         first / last non-silent frame on 63 | 64 and 255 | 256 | 257
                         `fmaxf(1e-10f, .)`                         all zeros; every mse below the floor; mse 1e-9 beside exact silence
                         `> -top_db`                                top_db = 0.5, 5, 20, 200

Guards: wav is a view into a NaN-filled buffer with 67 floats on either side (rows then start off 16-byte alignment), NaN past
each clip's own length; the table, out and the workspace are views into NaN-filled buffers, bounds into one filled with a negative
sentinel.  After every launch: the guards are intact, the inputs unchanged, every element of out finite and +0.0 by bit pattern
past ceil(len P / Q), every bounds pair written, every energy of a clip's own frames not NaN.  The bounds cases run a second time
over a workspace filled with a finite energy louder than any clip's: trim_bounds_kernel's fmaxf and comparisons drop a NaN, so a
frame read past a clip's own count shows only then.

Bounds, none tuned against the kernels:
  * exact probes: equality by bit pattern with int64 arithmetic (every product and partial sum an integer below 2^24).
  * production tables: tests/test_gpu_resample_trim.py's (2 W + 2) 2^-24 A + 1e-12 -- one rounding per coefficient and one per fmaf
    of the 2W-term chain, each at most 2^-24 of A = sum |x| |c|.
  * frame energies: (ceil(N / 64) + 8) 2^-24 mse -- a lane's chain of at most ceil(N / 64) fmaf roundings, six butterfly adds and
    one division, each at most 2^-24 of a partial sum, which is at most the sum itself since every term is non-negative.
  * trim bounds: equality with resample64.trim64 where every frame is at least 0.01 dB from the threshold, which the host test
    asserts of every case.

Largest error / bound measured on an MI355X (each test prints its own before it asserts; the module prints the table when it ends):
    resampler, (orig_sr, target_sr):  16000 -> 22050  0.069    48000 -> 22050  0.029    44100 -> 22050  0.036    11025 -> 22050  0.082
                                      22050 -> 16000  0.054    196 -> 185  0.060    185 -> 196  0.077    3 -> 2  0.042    2 -> 3  0.070
    frame energies, by N:             2  0.19    62  0.26    64  0.25    66  0.26    2048  0.057    8192  0.022    (largest: 0.26)
The bounds are worst-case sums of roundings; the kernels' errors add up like a random walk, hence the distance.  Every exact probe
and every bounds case passes, and no test here exposed a fault in csrc/resample.hip or its wrappers: nothing there was changed.
"""
import functools
import time
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio as Au  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import resample64 as R, resample_envelope as E  # noqa: E402

DEV = "cuda:0"
GUARD = 67
SENTINEL = -77
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print(f"\n[resample / trim envelope] largest error / bound per class: { {k: f'{v:.3e}' for k, v in WORST.items()} }; wall time {time.time() - t0:.1f} s")


def note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), float(worst))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def guarded(shape, dtype, host=None, fill=NAN):
    """(buffer, view of `shape` inside it): `fill` (int32: the sentinel) everywhere, the view holding `host` if there is one."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.int32 else fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if host is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return buf, view


def guards_hold(buf, n, fill=NAN):
    whole = buf.cpu().numpy()
    edge = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
    assert len(edge) == 2 * GUARD
    if whole.dtype == np.int32:
        return bool((edge == SENTINEL).all())
    return bool(np.isnan(edge).all()) if np.isnan(fill) else bool((edge == np.float32(fill)).all())


def untouched(buf):
    whole = buf.cpu().numpy()
    return bool((whole == SENTINEL).all()) if whole.dtype == np.int32 else bool(np.isnan(whole).all())


def poisoned(clips, L, lens=None):
    """(B, L) float32: row b holds the first lens[b] samples of clip b (all of it by default), NaN past them."""
    host = np.full((len(clips), L), np.nan, dtype=np.float32)
    for b, y in enumerate(clips):
        n = len(y) if lens is None else lens[b]
        host[b, :n] = np.asarray(y[:n], dtype=np.float32)
    return host


def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def raw_resample(host, lens, table, P, Q, W):
    """nsg_audio_resample on guarded buffers -> out (B, ceil(L_in P / Q)) numpy.  host (B, L_in) float32 with NaN past each clip;
    lens: None (a null pointer: every row is L_in long) or B integers for the device, used clamped into [0, L_in] as the header
    says the kernel does; table: the kernel's layout (2W, P)."""
    B, L_in = host.shape
    L_out = E.out_len(L_in, P, Q)
    assert table.shape == (2 * W, P) and table.dtype == np.float32
    wbuf, wav = guarded((B, L_in), torch.float32, host)
    tbuf, tab = guarded(table.shape, torch.float32, table)
    obuf, out = guarded((B, L_out), torch.float32)
    ld = None if lens is None else torch.tensor([int(n) for n in lens], dtype=torch.int32).to(DEV)
    _lib.call("nsg_audio_resample", _p(wav), _p(ld), _p(tab), _p(out), B, L_in, P, Q, W, _stream())
    torch.cuda.synchronize()
    for nm, buf, n in (("wav", wbuf, B * L_in), ("table", tbuf, table.size), ("out", obuf, B * L_out)):
        assert guards_hold(buf, n), f"a store outside {nm}"
    assert np.array_equal(bits(wav.cpu().numpy()), bits(host)) and np.array_equal(bits(tab.cpu().numpy()), bits(table)), "an input was written"
    o = out.cpu().numpy()
    assert np.isfinite(o).all(), "an output was not written, or a sample past a length (or outside the table) was read"
    for b in range(B):
        n = L_in if lens is None else clamp(lens[b], 0, L_in)
        assert not bits(o[b, E.out_len(n, P, Q):]).any(), f"row {b} is not +0.0 past its {E.out_len(n, P, Q)} samples"
    return o


LOUD_FILL = 3.0e38            # a finite energy louder than any clip's: fmaxf and the comparisons of trim_bounds_kernel drop a NaN


def raw_trim(host, lens, N, hop, top_db, fill=NAN):
    """nsg_audio_trim_bounds on guarded buffers with a workspace of exactly the queried size -> (bounds (B, 2), mse (B, T)) numpy.
    host (B, L) float32 with NaN past each clip; lens: None or B integers for the device, used clamped into [1, L].  fill: what
    the workspace holds before the launch, NaN or LOUD_FILL (an energy read past a clip's own frames is then the loudest)."""
    B, L = host.shape
    T = 1 + L // hop
    nb = _lib.query("nsg_audio_trim_workspace_bytes", B, L, hop)
    assert nb >= B * T * 4 and nb % 4 == 0
    wbuf, wav = guarded((B, L), torch.float32, host)
    sbuf, ws = guarded((nb // 4,), torch.float32, fill=fill)
    bbuf, bounds = guarded((B, 2), torch.int32)
    ld = None if lens is None else torch.tensor([int(n) for n in lens], dtype=torch.int32).to(DEV)
    _lib.call("nsg_audio_trim_bounds", _p(wav), _p(ld), _p(bounds), B, L, N, hop, float(top_db), _p(ws), nb, _stream())
    torch.cuda.synchronize()
    for nm, buf, n, f in (("wav", wbuf, B * L, NAN), ("the workspace", sbuf, nb // 4, fill), ("bounds", bbuf, 2 * B, NAN)):
        assert guards_hold(buf, n, f), f"a store outside {nm}"
    assert np.array_equal(bits(wav.cpu().numpy()), bits(host)), "the input was written"
    bd = bounds.cpu().numpy()
    assert (bd != SENTINEL).all(), "a bounds pair was not written"
    mse = ws.cpu().numpy()[:B * T].reshape(B, T)
    for b in range(B):
        n = L if lens is None else clamp(lens[b], 1, L)
        own = mse[b, :1 + n // hop]
        assert not np.isnan(own).any() and (own < LOUD_FILL).all(), f"clip {b}: an energy was not written, or a sample past its length was read"
        assert 0 <= bd[b, 0] <= bd[b, 1] <= n, (b, bd[b].tolist(), n)
    return bd, mse


# ----------------------------------------------------------------------------------------------------------------------
# resampler
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_case(P, Q, W, L_in):
    """[(name, rows (B, L_in) int64, table (P, 2W) int64, [want (L_out,) int64 per row])]: computed once."""
    lens = E.probe_lengths(P, Q, W, L_in)
    L_out = E.out_len(L_in, P, Q)
    seeded, distinct = E.probe_tables(P, Q, W)
    cases = []
    for name, rows, c in (("seeded", E.probe_samples(P, Q, W, L_in), seeded), ("comb", np.tile(E.impulse_comb(W, L_in), (len(lens), 1)), distinct)):
        cases.append((name, rows, c, [E.probe_ref(rows[b], n, c, P, Q, W, L_out)[0] for b, n in enumerate(lens)]))
    return cases


@pytest.mark.parametrize("P,Q,W,L_in", E.PROBE_GEOMETRIES)
def test_resampler_index_probe_is_exact(P, Q, W, L_in):
    """Integer samples and integer tables: the kernel equals the int64 double loop of the header's formula bit for bit, in one
    ragged launch and for each clip alone in a row of its own length (a null lengths pointer).  With the comb of unit impulses and
    the table of pairwise distinct entries, an output is the entry it used: its phase and its tap are read back from it."""
    lens = E.probe_lengths(P, Q, W, L_in)
    for name, rows, c, want in probe_case(P, Q, W, L_in):
        table = E.kernel_layout(c, Q).astype(np.float32)
        got = raw_resample(poisoned(rows, L_in, lens), lens, table, P, Q, W)
        for b, n in enumerate(lens):
            assert np.array_equal(bits(got[b]), bits(want[b].astype(np.float32))), (name, b, n, np.flatnonzero(got[b] != want[b])[:8].tolist())
            if name == "comb":
                m = np.flatnonzero(got[b])
                phase, tap = np.divmod(got[b][m].astype(np.int64) - 1, 2 * W)
                at = m * Q // P - W + 1 + tap
                assert np.array_equal(phase, (m * Q) % P) and (at >= 0).all() and (at < n).all() and rows[b][at].all(), (b, n)
                inside = np.arange(E.out_len(n, P, Q))
                reach = inside * Q // P
                assert set(inside[(reach - W + 1 >= 0) & (reach + W < n)]) <= set(m)          # a whole window inside the clip: never 0
            if n >= 1:
                alone = raw_resample(poisoned(rows[b:b + 1], n, [n]), None, table, P, Q, W)
            else:
                alone = raw_resample(poisoned(rows[b:b + 1], 1, [0]), [0], table, P, Q, W)
            assert np.array_equal(bits(alone[0]), bits(got[b, :alone.shape[1]])), (name, b, n)
            assert not got[b, alone.shape[1]:].any()
    print(f"{P} / {Q}, W = {W}, span {E.span_floats(P, Q, W)} floats: {len(lens)} lengths {lens}, L_out = {E.out_len(L_in, P, Q)}: exact")


@pytest.mark.parametrize("P,Q,W,L_in", [(3, 2, 2, 700), (2, 3, 3, 1200), (1, 64, 31, 64 * 300)])
def test_resampler_clamps_device_lengths_outside_the_row(P, Q, W, L_in):
    """lengths[b] = -5 is an empty clip (its row, all NaN, is never used), L_in + 9 is L_in (no read leaves the row)."""
    name, rows, c, _ = probe_case(P, Q, W, L_in)[0]
    table = E.kernel_layout(c, Q).astype(np.float32)
    dev_lens, eff = [-5, L_in + 9, 300, L_in + 9, -5], [0, L_in, 300, L_in, 0]
    got = raw_resample(poisoned(rows[:5], L_in, eff), dev_lens, table, P, Q, W)
    inside = raw_resample(poisoned(rows[:5], L_in, eff), eff, table, P, Q, W)
    assert np.array_equal(bits(got), bits(inside)) and not np.isnan(got).any()
    for b, n in enumerate(eff):
        want = E.probe_ref(rows[b], n, c, P, Q, W, got.shape[1])[0]
        assert np.array_equal(bits(got[b]), bits(want.astype(np.float32))), (b, n)
        assert n or not bits(got[b]).any()


@pytest.mark.parametrize("sr_in,sr_out", E.RATES + E.PITCH_RATIOS)
def test_production_tables_under_poison(sr_in, sr_out):
    """audio.resample_table's coefficients through the entry point on a ragged NaN-poisoned batch, against resample64 under the
    existing bound; each clip is bit for bit what audio.resample returns for it alone."""
    P, Q = R.ratio(sr_in, sr_out)
    W = R.half_width(P, Q)
    table = E.kernel_layout(Au.resample_table(P, Q), Q)
    clips, refs = E.production_case(sr_in, sr_out)
    lens = [len(x) for x in clips]
    got = raw_resample(poisoned(clips, max(lens) + 37), lens, table, P, Q, W)
    worst = 0.0
    for b, (x, (y64, A)) in enumerate(zip(clips, refs)):
        y = got[b, :len(y64)]
        e, bd = np.abs(y.astype(np.float64) - y64), E.resample_bound(sr_in, sr_out, A)
        worst = max(worst, float((e / bd).max()))
        print(f"{sr_in} -> {sr_out} ({P} / {Q}, W = {W}), {lens[b]} samples: max |y - y64| = {e.max():.3e}, max error / bound = {(e / bd).max():.3e}")
    print(f"{sr_in} -> {sr_out}: largest error / bound {worst:.3e}")
    note(f"resample {sr_in}->{sr_out}", worst)
    for b, (x, (y64, A)) in enumerate(zip(clips, refs)):
        y = got[b, :len(y64)]
        assert (np.abs(y.astype(np.float64) - y64) <= E.resample_bound(sr_in, sr_out, A)).all(), (sr_in, sr_out, lens[b])
        assert np.array_equal(bits(y), bits(Au.resample(x.copy(), sr_in, sr_out))), (sr_in, sr_out, lens[b])


def test_resampler_refusals_name_their_reason_and_write_nothing():
    """What tests/test_resample_host.py leaves: the message of each refusal, the LDS limit to the float (1 / 64 at W = 32 is one
    float over; W = 31 runs above), and the outputs, which keep their fill."""
    B, L_in = 2, 64
    wbuf, wav = guarded((B, L_in), torch.float32, np.ones((B, L_in), dtype=np.float32))
    tbuf, tab = guarded((2 * 65 * 8191,), torch.float32, np.zeros(2 * 65 * 8191, dtype=np.float32))        # the largest table named below
    obuf, out = guarded((B, 2 * L_in), torch.float32)

    def refused(match, B=B, L=L_in, up=3, down=2, W=2):
        with pytest.raises(_lib.NsgError, match=match):
            _lib.call("nsg_audio_resample", _p(wav), c_void_p(0), _p(tab), _p(out), B, L, up, down, W, _stream())
        torch.cuda.synchronize()
        assert untouched(obuf), match

    refused(r"4 / 2 is not in lowest terms", up=4, down=2)
    refused(r"1 / 64 needs 65540 bytes of LDS per tile, more than 64 KiB", up=1, down=64, W=32)
    refused(r"8191 / 8192 has 1064830 floats, more than 2\^20", up=8191, down=8192, W=65)
    for change in (dict(B=0), dict(B=-2), dict(L=0), dict(L=-64), dict(up=0), dict(up=-3), dict(down=0), dict(down=-2), dict(W=0), dict(W=-2)):
        refused(r"nsg_audio_resample: bad argument", **change)
    assert guards_hold(wbuf, B * L_in) and guards_hold(tbuf, 2 * 65 * 8191)


# ----------------------------------------------------------------------------------------------------------------------
# trimmer: frame energies
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.ENERGY_FRAMES)
def test_frame_energies_match_fp64(N):
    """Every frame t < 1 + len / hop of every clip against the fp64 mean(p^2) on trim64's padding, under E.energy_bound."""
    worst = 0.0
    rows = []
    for hop in E.energy_hops(N):
        clips = E.energy_clips(N, hop)
        lens = [len(y) for y in clips]
        bd, mse = raw_trim(poisoned(clips, max(lens) + 5), lens, N, hop, 20.0)
        for b, y in enumerate(clips):
            want = E.frame_mse64(y, N, hop)
            e = np.abs(mse[b, :len(want)].astype(np.float64) - want) / E.energy_bound(N, want)
            rows.append((hop, lens[b], float(e.max())))
            print(f"N = {N}, hop = {hop}, {lens[b]} samples, {len(want)} frames: max error / bound = {e.max():.3e}")
            b64, margin = R.trim64(y, 20.0, N, hop)
            if margin >= E.MARGIN_DB:
                assert tuple(bd[b]) == b64, (N, hop, b)
    worst = max(r[2] for r in rows)
    print(f"N = {N}: largest error / bound {worst:.3e}")
    note("frame energies", worst)
    note(f"frame energies N={N}", worst)
    for hop, n, e in rows:
        assert e <= 1.0, (N, hop, n, e)


@pytest.mark.parametrize("N,hop", E.EXACT_ENERGY)
def test_frame_energy_probe_is_exact(N, hop):
    """Integer samples in [-3, 3] and N a power of two: every sum of squares is an integer below 2^24 and the division exact, so
    the energy is the int64 sum over N by bit pattern, whatever the order of the adds."""
    clips = E.exact_energy_clips(N, hop)
    lens = [len(y) for y in clips]
    _, mse = raw_trim(poisoned(clips, max(lens) + 5), lens, N, hop, 20.0)
    for b, y in enumerate(clips):
        want = (E.frame_mse64(y, N, hop) / N).astype(np.float32)
        got = mse[b, :len(want)]
        assert np.array_equal(bits(got), bits(want)), (N, hop, b, np.flatnonzero(got != want)[:8].tolist())


# ----------------------------------------------------------------------------------------------------------------------
# trimmer: bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_length,hop,top_db", E.BOUNDS_LAUNCHES)
def test_trim_bounds_on_wave_and_round_boundaries(frame_length, hop, top_db):
    """Exact equality with trim64 (every case is at least 0.01 dB from the threshold: the host test asserts it, and so does this
    one), ragged in one launch with NaN past each length -- over a workspace of NaN, and again over one of energies louder than
    any clip's, which a frame read past a clip's own count would bring in (a NaN there is dropped by fmaxf and by the comparisons)
    -- then each clip alone in a row of its own length."""
    names, clips = E.bounds_launch(frame_length)
    want = []
    for name in names:
        b64, margin = E.bounds_ref(name, frame_length, hop, top_db)
        assert margin >= E.MARGIN_DB, (name, margin)
        want.append(b64)
    lens = [len(y) for y in clips]
    bd, _ = raw_trim(poisoned(clips, max(lens) + 3), lens, frame_length, hop, top_db)
    got = [tuple(r) for r in bd.tolist()]
    loud, _ = raw_trim(poisoned(clips, max(lens) + 3), lens, frame_length, hop, top_db, fill=LOUD_FILL)
    assert np.array_equal(loud, bd), "an energy past a clip's own frames was read"
    print("\n".join(f"[{frame_length}/{hop}, {top_db} dB] {nm}: {g} want {w}" for nm, g, w in zip(names, got, want)))
    assert got == want, [(nm, g, w) for nm, g, w in zip(names, got, want) if g != w]
    for name, y, w in zip(names, clips, want):
        alone, _ = raw_trim(poisoned([y], len(y)), None, frame_length, hop, top_db)
        assert tuple(alone[0].tolist()) == w, name
    for name in ("all_zeros", "below_the_floor"):
        assert got[names.index(name)] == (0, len(E.bounds_clips()[name][0]))


def test_trimmer_clamps_device_lengths_outside_the_row():
    """The header's stated behaviour when its precondition is broken: lengths below 1 and above L are used as 1 and L, nothing
    faults, no energy is NaN, and the bounds lie inside the row (raw_trim asserts 0 <= start <= end <= the clamped length)."""
    N, hop, L = 64, 16, 500
    rs = np.random.RandomState(9)
    dev_lens, eff = [0, -7, L + 9, L, 200, 1 << 30], [1, 1, L, L, 200, L]
    clips = [(0.3 * rs.randn(L)).astype(np.float32) for _ in eff]
    bd, mse = raw_trim(poisoned(clips, L, eff), dev_lens, N, hop, 20.0)
    assert (bd >= 0).all() and (bd <= L).all()
    inside, _ = raw_trim(poisoned(clips, L, eff), eff, N, hop, 20.0)
    assert np.array_equal(bd, inside)


def test_trimmer_refusals_name_their_reason_and_write_nothing():
    """What tests/test_resample_host.py leaves: the message of each refusal, the workspace limit to the byte, and the outputs,
    which keep their fill."""
    B, L, hop = 2, 96, 16
    nb = _lib.query("nsg_audio_trim_workspace_bytes", B, L, hop)
    wbuf, wav = guarded((B, L), torch.float32, np.ones((B, L), dtype=np.float32))
    sbuf, ws = guarded((nb // 4,), torch.float32)
    bbuf, bounds = guarded((B, 2), torch.int32)

    def refused(match, B=B, L=L, N=64, top_db=20.0, nbytes=nb):
        with pytest.raises(_lib.NsgError, match=match):
            _lib.call("nsg_audio_trim_bounds", _p(wav), c_void_p(0), _p(bounds), B, L, N, hop, top_db, _p(ws), nbytes, _stream())
        torch.cuda.synchronize()
        assert untouched(bbuf) and untouched(sbuf), match

    refused(r"frame_length must be even and in \[2, 8192\]", N=63)
    refused(r"frame_length must be even and in \[2, 8192\]", N=8194)
    refused(r"reflect padding needs more than frame_length/2 samples", L=32)
    refused(r"bad argument \(top_db > 0", top_db=0.0)
    refused(r"status -3\): nsg_audio_trim_bounds: workspace too small", nbytes=nb - 1)
    assert guards_hold(wbuf, B * L)
    bd, _ = raw_trim(np.ones((B, L), dtype=np.float32), None, 64, hop, 20.0)                  # and the same call with all of it runs
    assert bd.tolist() == [[0, L]] * B


# ----------------------------------------------------------------------------------------------------------------------
# composition
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num,den", [(196, 185), (185, 196)])
def test_pitch_shift_of_a_ragged_batch_is_tempo_then_resample_of_each_clip(num, den):
    P, Q = Au.resample_ratio(num, den)
    lens = [6000, 4097, den * 20, num * 20, 5003]
    rs = np.random.RandomState(num)
    clips = [(0.4 * np.sin(2 * np.pi * 180.0 * np.arange(n) / 22050) + 0.05 * rs.randn(n)).astype(np.float32) for n in lens]
    batch = torch.from_numpy(poisoned(clips, max(lens) + 11)).to(DEV)
    out, out_lens = Au.pitch_shift(batch, num, den, lengths=lens)
    assert out_lens.dtype == np.int32 and out_lens.tolist() == [E.out_len(n * num // den, P, Q) for n in lens]
    o = out.cpu().numpy()
    assert o.shape[1] >= out_lens.max() and np.isfinite(o).all()
    for b, y in enumerate(clips):
        alone = Au.resample(Au.tempo(y, float(den) / float(num)), num, den)
        assert len(alone) == out_lens[b] and np.array_equal(bits(o[b, :out_lens[b]]), bits(alone)), (num, den, b)
        assert not bits(o[b, out_lens[b]:]).any()
