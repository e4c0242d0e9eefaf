"""STOI's and ESTOI's four kernels (csrc/stoi.hip) across their envelope, against the fp64 restatement tests/helpers/stoi_ref.py
(whose conditions tests/test_stoi_envelope_host.py checks on the CPU) and exact identities.  A row of T frames has
L = 256 + 128 (T - 1) + r samples.  The boundaries, and the line of stoi.hip each belongs to:

    stoi_energy_kernel    `if (fr >= B * Tmax) return`              B * Tmax no multiple of 4: 1 x 1, 3 x 3, 6 x 513
                          `t >= stoi_frames(...)`: zeros            ragged lengths; Tmax floors (r = 77); 255 samples: no frame
    stoi_select_kernel    `for (t0 = 0; t0 < Tb; t0 += 256)`        T = 256 | 257 (one round | two), 512 | 513 (two full | a third)
                          `base += wcnt[0] + ...`                   speech with a dropped frame before 256 and a kept one after it;
                                                                    tones with kept = T on 256 | 257 | 512 | 513
                          `for (k = base + tid; k < Tmax; ...)`     the -1 tail: none (kept = Tmax), all (silence), in between
    stoi_envelope_kernel  `m >= 1 ? sb[m - 1] : -1`                 kept = 1: no neighbour at all; kept = 2: one on each side
                          `m + 1 < C ? sb[m + 1] : -1`              kept = Tmax in a row that is not the last: sb[m + 1] is then
                                                                    the NEXT clip's first frame, not a -1 of the tail or a guard
                          `if (m >= C)`: zeros                      rows past kept; a silent clip of full length
                          `r[(N - f) & (N - 1)]`                    f = 0 and f = 256 (they pair with themselves): band tables of
                                                                    one-bin bands [0, 1) .. [256, 257), and 15 runs over [0, 257)
    stoi_score_kernel     `C = C > Tmax ? Tmax : C`, `C < 30`       kept = 700 of 600, -3, 29 | 30 | 31
                          `for (i = tid; i < items; i += 256)`      STOI: segs * 15 = 255 | 270 (kept 46 | 47)
                          `for (s0 = 0; s0 < segs; s0 += 256)`      ESTOI: kept 285 | 286 (one tile | a refill), 541 | 542 (a third)
                          `nf = min(STOI_TILE_FRAMES, C - s0)`      NaN past kept: a frame the tile need not hold is never used
                          `fmin(alpha * yv, clip * xv)`             the clip binds (y = 10 x in a tenth of the frames)
                          `num / (sqrt(nx) * sqrt(ny) + EPS)`       nx == 0: a constant x envelope scores exactly 0.0

Guards: x and y are views into NaN-filled buffers (GUARD floats on either side), NaN past each clip's length; energy and env are
views into NaN-filled buffers, src and kept into buffers filled with a negative sentinel, so a read past a length poisons an
output, a missing store shows, and a store outside a tensor shows.  Every raw launch checks all six buffers.  The sentinel is
negative: a src read from a guard is then `no neighbour`, never an index.  Each test prints its figures before it asserts, and the
module prints its worst error / bound per class when it ends (pytest -s); DESIGN.md section 5l records them.

The ragged batch has six rows, one more than five lengths need: the silent clip of full length is a row of its own."""
import functools
import math
import time
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio as Au  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import stoi_ref as R  # noqa: E402

DEV = "cuda:0"
GUARD = 67
SENTINEL = -77
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print(f"\n[stoi envelope] worst error / bound per class: { {k: f'{v:.3e}' for k, v in WORST.items()} }; wall time {time.time() - t0:.1f} s")


def note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), float(worst))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def guarded(shape, dtype, host=None):
    """(buffer, view of `shape` inside it): NaN (int32: the sentinel) everywhere, the view holding `host` if there is one."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.int32 else NAN, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if host is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return buf, view


def guards_hold(buf, n):
    whole = buf.cpu().numpy()
    edge = np.concatenate([whole[:GUARD], whole[GUARD + n:]])
    assert len(edge) == 2 * GUARD
    return bool((edge == SENTINEL).all()) if whole.dtype == np.int32 else bool(np.isnan(edge).all())


def raw_envelopes(x, y, lens, bands=None):
    """nsg_audio_stoi_envelopes through the binding on guarded buffers, with the caller's band table -> numpy dict(energy (B, Tmax),
    src, kept, env (2, B, Tmax, 15)).  x, y (B, L) float32 on the host; everything past lens[b] is replaced by NaN; lens goes to the
    device.  The guards of all six buffers, the inputs themselves and `every element written` are checked here."""
    B, L = x.shape
    Tmax = R.n_frames(L)
    lens = np.asarray(lens, dtype=np.int32)
    past = np.arange(L)[None, :] >= lens[:, None]
    xin, yin = (np.where(past, np.float32(np.nan), a).astype(np.float32) for a in (x, y))
    xbuf, xd = guarded((B, L), torch.float32, xin)
    ybuf, yd = guarded((B, L), torch.float32, yin)
    ld = torch.from_numpy(lens).to(DEV)
    ebuf, energy = guarded((B, Tmax), torch.float64)
    sbuf, src = guarded((B, Tmax), torch.int32)
    kbuf, kept = guarded((B,), torch.int32)
    vbuf, env = guarded((2, B, Tmax, R.BANDS), torch.float32)
    table = np.ascontiguousarray(Au.stoi_bands() if bands is None else bands, dtype=np.int32)
    lo, hi = np.ascontiguousarray(table[:, 0]), np.ascontiguousarray(table[:, 1])
    _lib.call("nsg_audio_stoi_envelopes", _p(xd), _p(yd), _p(ld), c_void_p(lo.ctypes.data), c_void_p(hi.ctypes.data), _p(energy), _p(src), _p(kept),
              _p(env), B, L, _stream())
    torch.cuda.synchronize()
    for nm, buf, n in (("x", xbuf, B * L), ("y", ybuf, B * L), ("energy", ebuf, B * Tmax), ("src", sbuf, B * Tmax), ("kept", kbuf, B),
                       ("env", vbuf, 2 * B * Tmax * R.BANDS)):
        assert guards_hold(buf, n), f"a store outside {nm}"
    assert np.array_equal(bits(xd.cpu().numpy()), bits(xin)) and np.array_equal(bits(yd.cpu().numpy()), bits(yin)), "an input was written"
    out = dict(energy=energy.cpu().numpy(), src=src.cpu().numpy(), kept=kept.cpu().numpy(), env=env.cpu().numpy())
    assert not np.isnan(out["energy"]).any(), "an energy was not written, or a sample past a length was read"
    assert not np.isnan(out["env"]).any(), "an envelope was not written, or a sample past a length was read"
    assert (out["src"] != SENTINEL).all() and (out["kept"] != SENTINEL).all(), "an element of src or kept was not written"
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 restatement of every clip of a case, computed once and never changed."""
    x, y, lens, _ = R.envelope_batch(name)
    Tmax = R.n_frames(x.shape[1])
    return [R.envelopes64(x[b], y[b], int(lens[b]), Tmax) for b in range(len(lens))]


@functools.lru_cache(maxsize=None)
def launched(name):
    """The GPU's outputs for a case, launched once for the tests that share it."""
    x, y, lens, _ = R.envelope_batch(name)
    return raw_envelopes(x, y, lens)


def check_first_stage(got, ref, tag, bands=None):
    for b, r in enumerate(ref):
        assert r["margin_db"] >= 0.01, (tag, b)
        rel = np.abs(got["energy"][b] - r["energy"]) / np.where(r["energy"] > 0.0, r["energy"], 1.0)
        print(f"[{tag} clip {b}] worst |energy - energy_ref| / energy_ref = {rel.max():.3e}")
        note("energy", rel.max() / 1e-12)
        np.testing.assert_allclose(got["energy"][b], r["energy"], rtol=1e-12, atol=0.0)          # fp64 in another order
        assert got["kept"][b] == r["kept"], (tag, b, int(got["kept"][b]), r["kept"])
        assert np.array_equal(got["src"][b], r["src"]), (tag, b, int((got["src"][b] != r["src"]).sum()))       # the -1 tail included
        note("env", R.check_env(got["env"][:, b], r, f"{tag} clip {b}", bands=bands))


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the first stage across the frame-count boundaries
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ENVELOPE_CASES))
def test_first_stage_across_the_frame_counts(name):
    """T = 1; T = 2, 3 with B * Tmax = 9; T = 256 | 257 | 512 | 513, a tone (kept = T) in row 0 and speech with pauses in row 1;
    the ragged batch of 513, 257, 256 (r = 77), 30 and 0 frames and a silent clip of full length, in one launch."""
    x, _, lens, kinds = R.envelope_batch(name)
    got, ref = launched(name), reference(name)
    Tmax = R.n_frames(x.shape[1])
    assert got["env"].shape == (2, len(lens), Tmax, 15) and got["energy"].shape == got["src"].shape == (len(lens), Tmax)
    print(f"[{name}] B = {len(lens)}, L = {x.shape[1]}, Tmax = {Tmax}, kept = {got['kept'].tolist()}")
    check_first_stage(got, ref, name)
    for b, (kind, r) in enumerate(zip(kinds, ref)):
        T = R.n_frames(int(lens[b]))
        assert not got["energy"][b, T:].any() and (got["src"][b, r["kept"]:] == -1).all() and not got["env"][:, b, r["kept"]:].any()
        if kind == "tone":
            assert got["kept"][b] == T and np.array_equal(got["src"][b, :T], np.arange(T))
        if kind == "zero":
            assert got["kept"][b] == 0 and not got["energy"][b].any()


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. band tables that reach the spectrum's ends
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["one_bin", "full"])
def test_band_tables_that_reach_bins_0_and_256(table):
    """One-bin bands hold |X[0]|, |X[256]|, |Y[0]|, |Y[256]| each alone (bands 0 and 14); 15 runs cover every bin of [0, 257).
    Clips of 3 and of 40 frames with a DC offset and a component at 5 kHz."""
    bands = R.ONE_BIN_BANDS if table == "one_bin" else R.FULL_BANDS
    x, y, lens = R.band_batch()
    Tmax = R.n_frames(x.shape[1])
    ref = [R.envelopes64(x[b], y[b], int(lens[b]), Tmax, bands=bands) for b in range(2)]
    got = raw_envelopes(x, y, lens, bands)
    check_first_stage(got, ref, table, bands=bands)
    default = raw_envelopes(x, y, lens)
    for k in ("energy", "src", "kept"):                                                          # the table touches the envelopes alone
        assert np.array_equal(bits(got[k]), bits(default[k])), k
    if table == "one_bin":
        for b, r in enumerate(ref):
            C = r["kept"]
            ends = got["env"][:, b, :C][:, :, [0, 14]]
            print(f"[one_bin clip {b}] least |.| at bins 0 and 256 = {ends.min():.4f}, spectral peak {r['peak'].max():.4f}")
            assert ends.min() >= 0.1 * r["peak"].max()


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. exact probes
# ----------------------------------------------------------------------------------------------------------------------------------
def test_power_of_two_scaling_is_exact():
    """x, y scaled by 2^k, k = -8, +8: every operation of the first stage is a product or a sum of scaled terms (the twiddles and the
    window are the same numbers, sqrtf of 4^k a is 2^k sqrtf a) and nothing underflows at these sizes, so energy is exactly 4^k
    times, kept and src the same, env 2^k times bit for bit.  tests/test_stoi_envelope_host.py holds the same on env32_paired."""
    x, y, lens = R.scale_batch()
    base = raw_envelopes(x, y, lens)
    assert base["kept"].tolist() == [R.envelopes64(x[b], y[b], int(lens[b]))["kept"] for b in range(2)] and base["env"].any()
    for k in R.SCALE_POWERS:
        s = np.float32(2.0 ** k)
        got = raw_envelopes(x * s, y * s, lens)
        assert np.array_equal(bits(got["energy"]), bits(base["energy"] * 4.0 ** k)), k
        assert np.array_equal(got["kept"], base["kept"]) and np.array_equal(got["src"], base["src"]), k
        diff = int((bits(got["env"]) != bits(base["env"] * s)).sum())
        print(f"[2^{k}] envelopes that are not 2^{k} times the unscaled bits: {diff}")
        assert diff == 0, k


def test_long_clips_are_what_they_are_alone_and_a_second_launch_agrees():
    """The ragged batch of 513 frames: two launches give the same bits, and every clip alone in a row of its own length (the clip of
    255 samples: a row of 256) is its row of the batch in all four outputs."""
    x, y, lens, _ = R.envelope_batch("ragged")
    first = launched("ragged")
    again = raw_envelopes(x, y, lens)
    for k in ("energy", "src", "kept", "env"):
        assert np.array_equal(bits(first[k]), bits(again[k])), k
    for b, n in enumerate(lens):
        n = int(n)
        L1 = max(n, R.FRAME)
        one = raw_envelopes(x[b:b + 1, :L1], y[b:b + 1, :L1], [n])
        T1 = R.n_frames(L1)
        assert one["kept"][0] == first["kept"][b], b
        assert np.array_equal(bits(one["energy"][0]), bits(first["energy"][b, :T1])) and not first["energy"][b, T1:].any(), b
        assert np.array_equal(one["src"][0], first["src"][b, :T1]) and (first["src"][b, T1:] == -1).all(), b
        assert np.array_equal(bits(one["env"][:, 0]), bits(first["env"][:, b, :T1])) and not first["env"][:, b, T1:].any(), b


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. the score stage on synthetic envelopes
# ----------------------------------------------------------------------------------------------------------------------------------
def run_score(env, kept, extended):
    """audio.stoi_score on guarded views of env and kept -> d as numpy."""
    vbuf, ed = guarded(env.shape, torch.float32, env)
    kbuf, kd = guarded(kept.shape, torch.int32, kept)
    d = Au.stoi_score(ed, kd, extended)
    assert d.dtype == torch.float64 and tuple(d.shape) == kept.shape
    d = d.cpu().numpy()
    assert guards_hold(vbuf, env.size) and guards_hold(kbuf, kept.size)
    assert np.array_equal(bits(ed.cpu().numpy()), bits(env)) and np.array_equal(kd.cpu().numpy(), kept), "an input was written"
    return d


def test_score_stage_on_synthetic_envelopes_across_its_boundaries():
    """One launch, Tmax = 600, kept = 29, 30, 31, 46, 47, 285, 286, 541, 542, 600, 700 (clamped to 600) and -3, NaN past each kept.
    fp64 against fp64 on a quantity in [-1, 1]: 1e-10 absolute, NaN exactly where the reference gives NaN.  On the reference: every
    30-vector's standard deviation is at least 0.05 of its mean, and the -15 dB clip binds in every scored clip."""
    env, kept = R.score_case()
    for extended in (False, True):
        d = run_score(env, kept, extended)
        for b, k in enumerate(kept):
            C = R.clamp_kept(k, R.SCORE_TMAX)
            want = R.score64(env[:, b], C, extended)
            assert math.isnan(d[b]) == math.isnan(want) == (C < 30), (b, int(k), extended, d[b])
            if C >= 30:
                if not extended:
                    assert R.clip_binds(env[:, b], C) >= 1 and R.spread(env[:, b], C) >= R.MIN_SPREAD, b
                err = abs(d[b] - want)
                note("score", err / R.SCORE_TOL)
                print(f"[{'estoi' if extended else 'stoi'} kept {int(k)}] d = {d[b]:.12f}, |d - d64| = {err:.3e}, / bound = {err / R.SCORE_TOL:.3e}")
                assert err <= R.SCORE_TOL, (b, int(k), extended, d[b], want)
        assert np.array_equal(bits(d), bits(run_score(env, kept, extended)))


def test_score_stage_exact_cases():
    """Clip 0: env_x = 1.0 everywhere.  Its sums 30 x 1.0 and the mean 30 / 30 are exact, so every deviation of x is 0.0, every
    numerator 0.0 and every denominator at least eps: d is exactly 0.0 for both variants (ESTOI: the row-normalised x is 0.0 times
    a finite 1 / (0 + eps)).  Clip 1: env_y == env_x, conditioned as above.  STOI: alpha = sqrt(s / (s + eps)) is within 2^-52 of 1,
    alpha x is below clip x, and a vector's correlation with a positive multiple of itself is 1 up to eps / (nx ny)^(1/2) and a few
    roundings of 2^-53 per sum of 30.  ESTOI: x~ and y~ are the same numbers, so each column adds n^2 / (n + eps)^2 with n about 0.7.
    Both within 1e-12 of 1.  Kept = 290: ESTOI's second tile is met as well."""
    env, kept = R.exact_case()
    for extended in (False, True):
        d = run_score(env, kept, extended)
        print(f"[{'estoi' if extended else 'stoi'}] constant x: d = {d[0]!r}; y == x: d - 1 = {d[1] - 1.0:.3e}")
        assert d[0] == 0.0, (extended, d[0])
        assert abs(d[1] - 1.0) <= 1e-12, (extended, d[1])
        note("score y == x", abs(d[1] - 1.0) / 1e-12)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. end to end on the long clips
# ----------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_long_ragged_batch():
    """audio.stoi at 10 kHz against score64(envelopes64) on the ragged batch of 513 frames, both variants: |d - d_ref| <= TOL_FACTOR *
    DELTA.  This batch's own delta, reference against reference, is 5.12e-5 (tests/helpers/stoi_ref.py says how it is measured;
    tests/test_stoi_envelope_host.py measures it again), below DELTA = 9e-5, so DELTA itself is the bound."""
    x, y, lens, _ = R.envelope_batch("ragged")
    ref = reference("ragged")
    xd, yd = (torch.from_numpy(a).to(DEV) for a in (x, y))
    worst = 0.0
    for extended in (False, True):
        d, kept = Au.stoi(xd, yd, 10000, lens, extended)
        assert kept.tolist() == [r["kept"] for r in ref]
        d = d.cpu().numpy()
        for b, r in enumerate(ref):
            want = R.score64(r["env"], r["kept"], extended)
            assert math.isnan(d[b]) == math.isnan(want) == (r["kept"] < 30), (b, extended)
            if not math.isnan(want):
                ratio = abs(d[b] - want) / (R.TOL_FACTOR * R.DELTA)
                worst = max(worst, ratio)
                print(f"[{'estoi' if extended else 'stoi'} clip {b}, kept {r['kept']}] d = {d[b]:.9f}, ref {want:.9f}, |diff| / bound = {ratio:.3e}")
    note("end to end", worst)
    print(f"worst |d - d_ref| / ({R.TOL_FACTOR:g} * {R.DELTA:g}) = {worst:.3e}")
    assert worst <= 1.0
