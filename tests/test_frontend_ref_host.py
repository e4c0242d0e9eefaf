"""tests/helpers/frontend_ref64.py held to the older helpers it generalises, its case tables held to the edges the GPU module
relies on, its exact probes held to their exactness conditions, and its comparison rules held to planted errors -- all on the
CPU, with the reference alone (tests/test_gpu_frontend_envelope.py holds the kernels to the reference)."""
import math

import numpy as np
import pytest

from neural_sound_generation_amd import audio as Au
from tests.helpers import frontend_ref64 as R, mel_forward64 as H, resample64 as R64

MEL = R.mel_cases()


def _family(name):
    return [c for c in MEL if c.family == name]


# ---- the restatements against the helpers they generalise ------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,n_mels", [(1024, 256, 80), (512, 128, 40), (2048, 512, 80)])
def test_mel64_at_the_defaults_is_forward64(n_fft, hop, n_mels):
    y = H.signals(hop * 19)["harmonic"]
    out, m, xmax, rows = H.forward64(y, n_fft, hop, n_mels)
    r = R.mel64(y, len(y), Au.mel_basis(H.SR, n_fft, n_mels), Au._mel_bands(H.SR, n_fft, n_mels), n_fft, hop, 0.97, -100.0, 20.0, 1.0)
    assert r.out.shape == out.shape == (n_mels, 20) and r.Tb == r.T == 20
    assert np.abs(r.m - m).max() <= 1e-12 * max(1.0, m.max()) and abs(r.X.max() - xmax) <= 1e-12 * xmax
    assert np.abs(r.out - out).max() <= 1e-12 and np.abs(r.rows - rows).max() <= 1e-12
    m_inv, lo, hi = R.amplitude_of(out, -100, 20, 1)
    assert np.abs(m_inv - H.amplitude_of(out)).max() <= 1e-12 * m_inv.max() and math.isclose(lo, H.OUT_LO_AMP) and math.isclose(hi, H.OUT_HI_AMP)


@pytest.mark.parametrize("sr_in,sr_out", [(16000, 22050), (48000, 22050), (22050, 8000)])
def test_resample_sum_on_a_real_table_is_resample64(sr_in, sr_out):
    P, Q = R64.ratio(sr_in, sr_out)
    W = R64.half_width(P, Q)
    s = min(1.0, P / Q)
    c = s * R64.h(s * (np.arange(P)[:, None] / P + (W - 1 - np.arange(2 * W))[None, :]))        # nsg.h: c[phi][j]
    table = c[(np.arange(P) * Q) % P].T                                                        # table[j][k] = c[(k Q) mod P][j]
    assert np.abs(table - np.asarray(Au._resample_table_on(P, Q, "cpu"))).max() <= 2.0 ** -24
    x = np.random.RandomState(1).uniform(-1, 1, 1500)
    for length in (1, 50, 777, 1500):
        got, mag = R.resample_sum(x, length, table, P, Q, W, dtype=np.float64)
        want, A = R64.resample64(x[:length], sr_in, sr_out)
        n = len(want)
        assert n == R.cdiv(length * P, Q) and len(got) == R.cdiv(1500 * P, Q)
        assert np.abs(got[:n] - want).max() <= 1e-12 and np.abs(mag[:n] - A).max() <= 1e-12 and not got[n:].any()


def test_frame_energy_sums_are_trim64s():
    N, hop, clips, want = R.trim_block_batch()
    for y, (first, last) in zip(clips[:3], want[:3]):
        e = R.frame_energy_sums(y, len(y), N, hop)
        p = np.pad(y.astype(np.float64), N // 2, mode="reflect")
        assert all(e[t] == np.sum(p[t * hop:t * hop + N] ** 2) for t in range(0, len(e), 37))
        db = 10 * np.log10(np.maximum(1e-10, e / N)) - 10 * np.log10(e.max() / N)
        loud = np.flatnonzero(db > -R.TOP_DB)
        assert (loud[0], loud[-1]) == (first, last)


# ---- every edge is in a table ----------------------------------------------------------------------------------------------------
def test_mel_tables_hit_every_edge():
    assert {c.n_fft for c in _family("spectrum")} == set(R.MEL_NFFTS)
    for c in _family("spectrum"):
        basis, bands, names = R.basis_of(c)
        F = c.n_fft // 2 + 1
        assert basis.shape == (len(names), F) and len(names) <= R.MEL_MAX_ROWS
        single = {tuple(b) for b in bands.tolist() if b[0] == b[1]}
        assert {(0, 0), (1, 1), (F - 2, F - 2), (F - 1, F - 1)} <= single
        assert [0, F - 1] in bands.tolist() and any(b[0] > b[1] for b in bands.tolist())
        assert sum(n.startswith("run") for n in names) >= 3
        inside = (np.arange(F)[None, :] >= bands[:, :1]) & (np.arange(F)[None, :] <= bands[:, 1:])
        assert (basis[~inside] == R.OUTSIDE).all() and (basis[inside] >= 0).all() and basis[inside].max() < 1.0
        assert (bands >= 0).all() and (bands < F).all()                      # an empty row's indices are legal ones too
        assert c.kinds == ["noise", "dc", "nyquist", "sine"]
    hops = {(c.n_fft, c.hop) for c in _family("hop")}
    assert hops == {(N, h) for N in R.MEL_NFFTS for h in (1, 100, N // 8, N // 4, N // 2 + 1, N, N + 37)}
    assert all(c.T <= 20 or c.hop == 1 for c in _family("hop")) and all(c.lens == [c.n_fft // 2 + 1] for c in _family("hop") if c.hop == 1)
    assert {(c.n_fft, c.lens[0]) for c in _family("length")} == {(N, N // 2 + d) for N in R.MEL_NFFTS for d in (1, 2)}
    assert R.parity_combinations(_family("parity")) == {(0, 0, False), (1, 1, False), (0, 0, True), (0, 1, True), (1, 0, True), (1, 1, True)}
    assert [c.basis for c in _family("rows")] == [1, 2, R.MEL_MAX_ROWS - 1, R.MEL_MAX_ROWS]
    assert [c.params for c in _family("params")] == [(0.97, -100.0, 20.0, 1.0), (0.0, -80.0, 0.0, 4.0), (-0.5, -100.0, -20.0, 1.0), (1.0, -60.0, 20.0, 0.5)]
    assert {(c.n_fft, c.kinds[0]) for c in _family("leak")} == {(N, kind) for N in R.MEL_NFFTS for kind in ("loud_odd", "loud_even")}
    assert all(c.hop == c.n_fft and c.params[0] == 0.0 for c in _family("leak"))


def test_the_signals_reach_the_bins_and_the_clips_they_are_for():
    """White noise clips nowhere on the single-bin and small-weight rows (so the full sensitivity of the bound applies there);
    the DC / Nyquist clips put their energy on the DC / Nyquist single-bin row, unclipped; every parameter set clips entries at
    both ends; the floor of the third set comes out at 0.2; in the leak cases the quiet frames are exact zeros."""
    for c in _family("spectrum"):
        basis, bands, names = R.basis_of(c)
        wav = R.mel_wav(c)
        _, lo, hi = R.amplitude_of(0.0, *c.params[1:])
        for b, kind in enumerate(c.kinds):
            r = R.mel64(wav[b], c.lens[b], basis, bands, c.n_fft, c.hop, *c.params)
            if kind == "noise":
                keep = [j for j, n in enumerate(names) if n not in ("hot", "empty")]
                assert (r.m[keep] > lo).mean() > 0.95 and (r.m[keep] < hi / 2).all()
                assert (r.m[names.index("hot")] > hi).all()
            if kind in ("dc", "nyquist"):
                j = names.index("bin0" if kind == "dc" else "binN/2")
                assert (r.m[j] > 10 * lo).all() and (r.m[j] < hi / 2).all() and r.X.argmax(axis=0).tolist() == [bands[j, 0]] * r.Tb
            if kind == "sine":
                assert set(r.X[:, 2:-2].argmax(axis=0).tolist()) == {c.n_fft // 8 + 1}
    for c in _family("params"):
        basis, bands, names = R.basis_of(c)
        r = R.mel64(R.mel_wav(c)[0], c.lens[0], basis, bands, c.n_fft, c.hop, *c.params)
        _, lo, hi = R.amplitude_of(0.0, *c.params[1:])
        live = [j for j, n in enumerate(names) if n != "empty"]
        assert (r.m[live] <= lo).any() and (r.m >= hi).any() and ((r.m > lo) & (r.m < hi)).sum() > r.m.size // 8
    assert abs(R.floor_value(*R.PARAM_SETS[2][1:])[0] - 0.2) < 1e-8
    assert [R.floor_value(*p[1:])[0] for p in (R.PARAM_SETS[0], R.PARAM_SETS[1], R.PARAM_SETS[3])] == [0.0, 0.0, 0.0]
    for c in _family("leak"):
        basis, bands, names = R.basis_of(c)
        r = R.mel64(R.mel_wav(c)[0], c.lens[0], basis, bands, c.n_fft, c.hop, *c.params)
        quiet = slice(0, None, 2) if c.kinds[0] == "loud_odd" else slice(1, None, 2)
        loud = slice(1, None, 2) if c.kinds[0] == "loud_odd" else slice(0, None, 2)
        assert r.Tb == 8 and not r.X[:, quiet].any() and (r.X[:, loud].max(axis=0) > 1.0).all()


def test_preemphasis_and_resampler_tables_hit_every_edge():
    assert [L for B, L in R.PRE_SHAPES if B == 5] == [1, 2, 255, 256, 257] and R.PRE_KS == (0.0, 0.97, -0.5, 1.0)
    B, L = R.PRE_SHAPES[-1]
    assert B == 3 and R.EW_BLOCKS * R.EW_THREADS < B * L <= R.EW_BLOCKS * R.EW_THREADS + B and L % R.EW_THREADS
    assert any(P == 1 for P, Q, W in R.RS_PROBES) and any(Q == 1 for P, Q, W in R.RS_PROBES)
    assert {W for P, Q, W in R.RS_PROBES if P > Q > 1} >= {1, 2, 3, 64} and {W for P, Q, W in R.RS_PROBES if 1 < P < Q and P < 100} >= {1, 2, 3, 64}
    assert {(441, 320, 64), (147, 640, 279), (1, 42, 2688)} <= set(R.RS_PROBES)
    for P, Q, W in R.RS_PROBES:
        assert math.gcd(P, Q) == 1 and P * 2 * W <= R.RS_MAX_TABLE and R.rs_lds_bytes(P, Q, W) <= R.RS_MAX_LDS
        L_in = R.rs_row(P, Q)
        L_out = R.cdiv(L_in * P, Q)
        tiles = R.cdiv(L_out, R.RS_TILE)
        assert tiles >= 4 and L_out % R.RS_TILE
        lens = R.rs_lengths(P, Q)
        assert lens[:2] == [0, 1] and lens[-1] == L_in and max(lens) == L_in
        for i, kth in enumerate((1, 2, tiles - 1)):
            a = lens[2 + 2 * i]
            assert lens[3 + 2 * i] == a + 1 and R.cdiv(a * P, Q) <= kth * R.RS_TILE < R.cdiv((a + 1) * P, Q)
        assert R.cdiv(R.cdiv(lens[-2] * P, Q), R.RS_TILE) <= tiles - 2                   # its last two tiles lie wholly past its end
        wav, shuffled, table = R.rs_probe(P, Q, W)
        assert sorted(shuffled) == sorted(lens) and shuffled != lens and wav.shape == (len(lens), L_in) and table.shape == (2 * W, P)
    assert R.rs_lds_bytes(1, 42, 2688) == 64348 and R.rs_lds_bytes(*R.RS_REFUSED_LDS) == 65880 > R.RS_MAX_LDS
    assert R.RS_REFUSED_LDS[0] * 2 * R.RS_REFUSED_LDS[2] <= R.RS_MAX_TABLE              # refused for the LDS, not for the table
    assert [(a, b) for a, b, _ in R.RS_ROUNDING] == [(22050, 8000), (96000, 22050), (42, 1)]
    assert all(2000 <= n <= 12000 for _, _, n in R.RS_ROUNDING)


def test_the_integer_probes_are_exact_in_fp32():
    """Every sum of |terms|, hence every partial sum in any order, stays below 2^24: fp32 arithmetic on them is exact."""
    for P, Q, W in R.RS_PROBES:
        wav, lens, table = R.rs_probe(P, Q, W)
        assert np.abs(wav).max() <= 8 and np.abs(table).max() <= 8 and (wav == np.rint(wav)).all() and (table == np.rint(table)).all()
        assert 8 * 8 * 2 * W < R.EXACT_SUM
        b = int(np.argmax(lens))
        out, mag = R.resample_sum(wav[b], lens[b], table, P, Q, W)
        assert 0 < mag.max() < R.EXACT_SUM and out.dtype == np.int64 and np.abs(out).max() > 8
    assert 15 * 15 * R.TRIM_MAX_FRAME < R.EXACT_SUM and max(N for N, _ in R.TRIM_SHAPES) == R.TRIM_MAX_FRAME


def test_trim_tables_hit_every_edge():
    assert set(R.TRIM_SHAPES) == {(2, 1), (64, 16), (512, 128), (2048, 512), (8192, 2048), (1000, 300), (64, 200)}
    N, hop, clips, want = R.trim_block_batch()
    assert (N, hop) == (64, 16)
    frames = [1 + len(y) // hop for y in clips]
    assert min(frames) >= 900 and max(frames) <= 1100 and len(set(frames)) > 5
    assert {f for f, _ in want} == {255, 256, 257, 600}
    assert {l for l, _ in zip([w[1] for w in want], want)} >= {511, 512} and any(l == T - 1 for (_, l), T in zip(want, frames))
    for y, (first, last) in zip(clips, want):
        assert np.abs(y).max() <= 15 and (y == np.rint(y)).all()
        e = R.frame_energy_sums(y, len(y), N, hop).astype(np.float64)
        db = 10 * np.log10(np.maximum(1e-10, e / N)) - 10 * np.log10(e.max() / N)
        inside = np.zeros(len(e), bool)
        inside[first:last + 1] = True
        assert (db[inside] > -R.TOP_DB + 5).all() and (db[~inside] <= -30.0).all() and (~inside).sum() > 200
        (start, end), margin = R64.trim64(y, R.TOP_DB, N, hop)
        assert margin >= 0.01 and (start, end) == (first * hop, min(len(y), (last + 1) * hop))
    for N, hop in R.TRIM_SHAPES:
        mid, short, zero = R.trim_shape_batch(N, hop)
        assert len(short) == N // 2 + 1 and (1 + len(short) // hop == 1) == (hop > len(short)) and not zero.any() and len(zero) > N // 2
        e = R.frame_energy_sums(mid, len(mid), N, hop).astype(np.float64)
        db = 10 * np.log10(np.maximum(1e-10, e / N)) - 10 * np.log10(e.max() / N)
        assert (db[6:14] > -R.TOP_DB + 5).all() and (np.delete(db, np.arange(6, 14)) <= -30.0).all()
        assert R64.trim64(mid, R.TOP_DB, N, hop)[0] == (6 * hop, 14 * hop)
        assert R64.trim64(zero, R.TOP_DB, N, hop)[0] == (0, len(zero)) and R64.trim64(short, R.TOP_DB, N, hop)[0] == (0, len(short))


# ---- the rules reject planted errors -----------------------------------------------------------------------------------------------
def _spectrum_ref(n_fft, b):
    c = [c for c in _family("spectrum") if c.n_fft == n_fft][0]
    basis, bands, names = R.basis_of(c)
    x = R.mel_wav(c)[b]
    return c, basis, bands, names, x, R.mel64(x, c.lens[b], basis, bands, c.n_fft, c.hop, *c.params)


def _rejected(out, c, basis, bands, x, length, ref):
    try:
        R.check_mel(out.astype(np.float32), x, length, basis, bands, c.n_fft, c.hop, *c.params, ref=ref, quiet=True)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("n_fft", R.MEL_NFFTS)
def test_check_mel_rejects_planted_errors(n_fft):
    for b, f_bad in ((0, 0), (0, n_fft // 2), (1, 0), (2, n_fft // 2)):            # noise, then the pure DC / Nyquist clips
        c, basis, bands, names, x, ref = _spectrum_ref(n_fft, b)
        assert not _rejected(ref.out, c, basis, bands, x, c.lens[b], ref), "the reference itself (rounded to fp32) passes"
        X = ref.X.copy()
        X[f_bad, 1::2] *= 2.0                                                       # a DC / Nyquist bin doubled in the odd frames
        out = ref.out.copy()
        out[:, :ref.Tb] = R.normalise(R.band_matrix(basis, bands) @ X, *c.params[1:])
        assert _rejected(out, c, basis, bands, x, c.lens[b], ref), (b, f_bad)
        only = np.flatnonzero(np.abs(out - ref.out).max(axis=1) > 1e-6)
        assert set(only) <= {names.index(n) for n in ("bin0", "binN/2", "full", "hot")}     # the Slaney rows would not have seen it
    c, basis, bands, names, x, ref = _spectrum_ref(n_fft, 0)
    swapped = ref.out.copy()
    swapped[:, 2:4] = ref.out[:, [3, 2]]                                            # the two frames of a pair swapped
    assert _rejected(swapped, c, basis, bands, x, c.lens[0], ref)
    late = ref.out.copy()
    late[:, ref.Tb - 1] = 0.0                                                       # the last frame taken for padding
    assert _rejected(late, c, basis, bands, x, c.lens[0], ref)


def test_the_pair_bound_is_tighter_than_the_clip_bound():
    """An error of half the clip-wide delta in a frame whose pair is 50x quieter than the clip's loudest frame: inside the old
    rule (mel_forward64.check_amplitude's delta), outside the pair's."""
    c, basis, bands, names, x, _ = _spectrum_ref(512, 0)
    x = x.copy()
    x[:c.hop * 3] *= 0.02
    ref = R.mel64(x, c.lens[0], basis, bands, c.n_fft, c.hop, *c.params)
    j = names.index("full")
    m = ref.m.copy()
    out = ref.out.copy()
    clip_delta = R.REL * ref.X.max() * ref.rows[j]
    pair_delta = R.REL * R.pair_peak(ref.X)[0] * ref.rows[j]
    assert pair_delta < 0.1 * clip_delta
    m[j, 0] = ref.m[j, 0] + 0.5 * clip_delta                                        # inside the old rule, outside the new one
    out[:, :ref.Tb] = R.normalise(m, *c.params[1:])
    assert _rejected(out, c, basis, bands, x, c.lens[0], ref)


def test_the_exact_rules_reject_planted_errors():
    P, Q, W = 441, 320, 64
    wav, lens, table = R.rs_probe(P, Q, W)
    b = int(np.argmax(lens))
    want, _ = R.resample_sum(wav[b], lens[b], table, P, Q, W)
    R.assert_same(want.astype(np.float32), want)
    with pytest.raises(AssertionError):
        R.assert_same(np.roll(want, 1).astype(np.float32), want)                    # an output shifted by one sample
    later, _ = R.resample_sum(np.concatenate([[0], wav[b][:-1]]), lens[b], table, P, Q, W)      # `lo` off by one: the input shifted
    with pytest.raises(AssertionError):
        R.assert_same(later, want)
    N, hop, clips, frames = R.trim_block_batch()
    (start, end), _ = R64.trim64(clips[0], R.TOP_DB, N, hop)
    for bad in ((start + hop, end), (start, end - hop), (start - hop, end)):        # a trim bound off by one hop
        with pytest.raises(AssertionError):
            R.assert_same(np.array(bad), np.array((start, end)))
    # t += 512 in trim_bounds_kernel: the frames of every second pass are not seen
    e = R.frame_energy_sums(clips[0], len(clips[0]), N, hop)
    seen = (np.arange(len(e)) // R.TRIM_BLOCK) % 2 == 0
    db = 10 * np.log10(np.maximum(1e-10, e / N)) - 10 * np.log10(e[seen].max() / N)
    loud = np.flatnonzero((db > -R.TOP_DB) & seen)
    assert (loud[0] * hop, min(len(clips[0]), (loud[-1] + 1) * hop)) != (start, end)


# ---- calibration of the pair-peak bound without the kernel -------------------------------------------------------------------------
def test_fp32_paired_fft_restatement_sits_far_inside_the_bound():
    """mel32_paired (complex64 torch.fft.fft of both frames in one transform, fp32 throughout) through check_mel on EVERY mel
    case of the tables.  Recorded worst error / bound per family: spectrum 1.6e-2, hop 2.1e-2, length 8.5e-3, parity 1.0e-2,
    rows 2.0e-2, params 4.1e-2, leak 3.4e-2 -- the level of rounding the fp32 output alone (half an ulp of an output of 0.8 is
    3.4e-7 of its amplitude, 1.7e-2 of REL).  The gate is one quarter of the bound, so REL = 2e-5 of the PAIR's peak stays as it is
    and no constant had to be re-derived from the rounding count."""
    worst = {}
    for c in MEL:
        basis, bands, _ = R.basis_of(c)
        wav = R.mel_wav(c)
        for b in range(c.B):
            out = mel32 = R.mel32_paired(wav[b], c.lens[b], basis, bands, c.n_fft, c.hop, *c.params)
            _, w = R.check_mel(out[:, :1 + c.L // c.hop], wav[b], c.lens[b], basis, bands, c.n_fft, c.hop, *c.params, tag=c.tag, quiet=True)
            worst[c.family] = max(worst.get(c.family, 0.0), w)
            assert mel32.dtype == np.float32
    print("fp32 paired-FFT restatement, worst error / bound per family:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 0.25, worst


# ---- the refusals no small buffer reaches, with pointers that are never dereferenced ------------------------------------------------
def test_melspectrogram_refuses_2_31_frames_before_any_launch():
    """B * T >= 2^31 - 1 (tests/test_gpu_frontend_envelope.py has every refusal that small arguments reach; the resampler's and
    the trimmer's size limits are in tests/test_resample_host.py)."""
    import ctypes

    from neural_sound_generation_amd import _lib
    lib = _lib.load()
    ok = ctypes.c_void_p(0x10000)
    bands = np.zeros((4, 2), dtype=np.int32)

    def mel(B, L, hop):
        return lib.nsg_audio_melspectrogram(ok, None, ok, ctypes.c_void_p(bands.ctypes.data), ok, B, L, 512, hop, 4, 0.97, -100.0, 20.0, 1.0, 0, None)

    for B, L, hop in ((1 << 21, 1023, 1), (1 << 16, (1 << 15) - 1, 1), (0x7fffffff, 257, 258)):
        assert B * (1 + L // hop) >= 0x7fffffff
        assert mel(B, L, hop) == R.E_UNSUPPORTED, (B, L, hop)
        assert b"nsg_audio_melspectrogram: too many frames" in lib.nsg_last_error_string()
