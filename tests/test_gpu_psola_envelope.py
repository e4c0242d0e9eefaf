"""psola_marks_kernel, psola_syn_kernel and psola_ola_kernel (csrc/psola.hip) across their envelope, called at the C entry points
nsg_audio_pitch_marks and nsg_audio_psola so that the test chooses every launch constant, every buffer and the marks handed to the
second entry point.  Cases, signals, the ring simulation and the closed forms: tests/helpers/psola_envelope.py
(tests/test_psola_envelope_host.py proves on the CPU what they assume: that the ring-stress case reaches the 2048-sample step and
the 2559-sample reach the ring induction allows, that the long case wraps the period ring, that no case sits on the weight floor).
The boundaries, and the line of psola.hip each belongs to:

    psola_marks_kernel   `adv = lo >= (base + 1) * PS_H`             ring stress: a rising ramp, P = 1024, alpha 1/2, coin-flip voicing at
                                                                     hop 16 -- 14 advances, a stale or late half moves a maximum
                         `per[... & (PS_FR - 1)]`                    3 751 frames at hop 16 (three wraps, voicing differs between aliases);
                                                                     the long case: 1 172 frames at hop 256, 73 advances; the seam
                                                                     frame: a commit writes frame 768 while a mark at sample 4096
                                                                     still reads frame 256, 512 slots away and voiced otherwise
                         `ps_search`                                 ramps: the last / first sample of every range, by closed form
                         `nsg_div(g.an * pp, g.div_ad)`              alpha 0 / 1, 1 / 2 and 262143 / 2^20 (a product of 2^26 and more)
                         `ps_frame`, `tc = min(t, T - 1)`            hop 16 and 2^20, T = 1, a track shorter than the clip
                         `g.Pu = ps_clamp(Pu, Pmin, Pmax)`           P_u = 1 under P_min = 2, 5000 over P_max = 339
    psola_syn_kernel     `b = blockIdx.x * 64 + threadIdx.x`         130 ragged clips: three blocks, two live threads in the last
                         `r < 0.25 ? 0.25 : (r > 4.0 ? 4.0 : ...`    ratios exactly 0.25 and 4, their float32 neighbours, and exact ties
                         `while (j < J_max)`, `ps_marks`, `at()`     hostile marks and counts; G = 1 where K_max = J_max = L
    psola_ola_kernel     `n < n0 + PS_TILE && n < L`                 L = 1023, 1024, 1025, 2049
                         `sb[mid] > n - H_max`, `s >= n + H_max`     hostile marks further apart than H_max: the walk cuts the grain
                         `nsg_clip_len`                              lengths NULL, -5, L + 1000

Guards: wav, f0_in, f0_out, lengths, marks, n_marks, syn, map, n_syn and out are views into buffers with 67 elements on either side
(rows then start off 16-byte alignment), NaN around floats and a sentinel no kernel writes around integers; wav is NaN past each
clip's length; integer outputs are pre-filled with -2 and out with NaN.  After every launch: the guards are intact, the inputs
unchanged (the marks too, across nsg_audio_psola).  Every comparison is of whole rows, the -1 and +0.0 padding included.

Bounds, none tuned against the kernels: marks, counts, synthesis marks and map are integers and equal the restatement; out equals
the fp32 restatement by bit pattern and is within psola_ref.fp32_bound (a worst-case sum of the roundings) of the fp64 one, except
where the fp64 weight sum is within 1e-5 of the floor 2^-10 (the host test caps those samples at 0.1 % of a clip).  Each test prints
its largest error / bound before it asserts; the module prints the table when it ends.

Largest error / bound measured on an MI355X:
    widest  0.025    narrowest  0.002    alpha zero  0.014    big denominator  0.018    small hop  0.024    long  0.018
    one frame for all  0.011    T = 1  0.018    short track  0.020    P_u above  0.017    ring stress and the ramps  0.019
    L = 1023, 1024, 1025  0.022    L = 2049  0.017    130 clips  0.021    lengths NULL  0.021    ratio edges  0.010    (largest: 0.025)
The bound is a worst-case sum of roundings; the errors add up like a random walk, hence the distance.  Every case passes, and no
test here exposed a fault in csrc/psola.hip: nothing there was changed.  (Handing in marks further apart than H_max showed a rule
the header had left implied -- the overlap-add cuts a grain at |dist| < H_max -- which include/nsg.h and the restatement now state.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import psola_envelope as E, psola_ref as R  # noqa: E402

DEV = "cuda:0"
GUARD = 67
SENTINEL = -77                                         # around integer buffers: no mark, count or index is negative but -1
POISON = -2                                            # integer outputs before a launch
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\nlargest error / bound:  " + "    ".join(f"{k}  {v:.3f}" for k, v in WORST.items()))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Guarded:
    """A (rows, cols) view into a buffer with GUARD elements of `edge` on either side."""

    def __init__(self, name, host=None, shape=None, dtype=torch.float32, fill=None):
        shape = host.shape if host is not None else shape
        self.name, self.size, self.float = name, int(np.prod(shape)), dtype == torch.float32
        self.buf = torch.full((self.size + 2 * GUARD,), NAN if self.float else SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + self.size].view(*shape)
        if host is not None:
            self.view.copy_(torch.from_numpy(host))
        else:
            self.view.fill_(fill)
        self.host = host

    def read(self, unchanged=False):
        whole = self.buf.cpu().numpy()
        edge = np.concatenate([whole[:GUARD], whole[GUARD + self.size:]])
        assert (np.isnan(edge) if self.float else edge == SENTINEL).all(), f"a store outside {self.name}"
        got = whole[GUARD:GUARD + self.size].reshape(self.view.shape)
        if unchanged:
            assert np.array_equal(got.view(np.int32), self.host.view(np.int32)), f"{self.name} was written"
        return got


def launch(geo, clips, L=None, rows=None, B=None, K_extra=0, J_extra=0, lengths="own", marks=None):
    """Both entry points on the clips [(x, n, f0_in, f0_out)], clip i in row rows[i] of B rows of L samples: NaN past each clip's
    n, the other rows NaN and empty.  lengths: "own" (each clip's n), None (a NULL pointer) or (B,) raw device values.  marks:
    None (nsg_audio_pitch_marks' own) or (row (K_max,), count) per clip, handed to nsg_audio_psola instead -> dict of numpy arrays
    of the clips' rows, and what the restatement needs: the tracks as launched and the sizes."""
    rows = list(range(len(clips))) if rows is None else rows
    B = max(rows) + 1 if B is None else B
    L = max(1, max(len(c[0]) for c in clips)) if L is None else L
    T = max(1, max(len(c[2]) for c in clips))
    wav = np.full((B, L), np.nan, dtype=np.float32)
    lens = np.zeros(B, dtype=np.int32)
    fi, fo = np.zeros((B, T), dtype=np.float32), np.zeros((B, T), dtype=np.float32)
    for r, (x, n, a, b) in zip(rows, clips):
        n = max(0, min(int(n), len(x), L))
        wav[r, :n] = x[:n]
        lens[r] = n
        fi[r, :len(a)], fo[r, :len(b)] = a, b
        fi[r, len(a):], fo[r, len(b):] = a[-1], b[-1]                        # frames past a clip's own track: its last
    if lengths is None:
        assert (lens == L).all()
    elif not isinstance(lengths, str):
        lens = np.asarray(lengths, dtype=np.int32)
    _, K_max, H_max, _, J_max = R.sizes(L, geo.P_min, geo.P_max, geo.alpha)
    K_max, J_max = K_max + K_extra, J_max + J_extra
    I32 = torch.int32
    g_wav, g_fi, g_fo, g_len = Guarded("wav", wav), Guarded("f0_in", fi), Guarded("f0_out", fo), Guarded("lengths", lens, dtype=I32)
    g_marks, g_nm = Guarded("marks", shape=(B, K_max), dtype=I32, fill=POISON), Guarded("n_marks", shape=(B,), dtype=I32, fill=POISON)
    g_syn, g_map = Guarded("syn", shape=(B, J_max), dtype=I32, fill=POISON), Guarded("map", shape=(B, J_max), dtype=I32, fill=POISON)
    g_ns, g_out = Guarded("n_syn", shape=(B,), dtype=I32, fill=POISON), Guarded("out", shape=(B, L), fill=NAN)
    lens_p = _p(None) if lengths is None else _p(g_len.view)
    consts = (B, L, T, geo.hop, float(geo.sr), geo.P_u, geo.P_min, geo.P_max, geo.alpha[0], geo.alpha[1], K_max)
    if marks is None:
        _lib.call("nsg_audio_pitch_marks", _p(g_wav.view), lens_p, _p(g_fi.view), _p(g_marks.view), _p(g_nm.view), *consts, _stream())
        g_marks.host, g_nm.host = g_marks.read(), g_nm.read()
    else:
        m, c = np.full((B, K_max), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
        for r, (row, count) in zip(rows, marks):
            m[r, :len(row)], c[r] = row, count
        g_marks, g_nm = Guarded("marks", m, dtype=I32), Guarded("n_marks", c, dtype=I32)
    _lib.call("nsg_audio_psola", _p(g_wav.view), lens_p, _p(g_fi.view), _p(g_fo.view), _p(g_marks.view), _p(g_nm.view), _p(g_syn.view),
              _p(g_map.view), _p(g_ns.view), _p(g_out.view), *consts, J_max, _stream())
    torch.cuda.synchronize()
    for g in (g_wav, g_fi, g_fo, g_len):
        g.read(unchanged=True)
    res = dict(marks=g_marks.read(unchanged=True), n_marks=g_nm.read(unchanged=True), syn=g_syn.read(), map=g_map.read(), n_syn=g_ns.read(),
               out=g_out.read())
    res = {k: v[rows] for k, v in res.items()}
    res.update(f0_in=fi[rows], f0_out=fo[rows], L=L, K_max=K_max, J_max=J_max, H_max=H_max, handed=marks)
    return res


def check(geo, clips, got, fp64=True, name=None):
    """Row i of `got` against the restatement of clip i, whole rows: the -1 and +0.0 padding included -> largest error / bound."""
    L, worst = got["L"], 0.0
    pad = lambda v, m: np.concatenate([np.asarray(v, dtype=np.int32), np.full(m - len(v), -1, dtype=np.int32)])
    for i, (x, n, _, _) in enumerate(clips):
        x = np.asarray(x[:L], dtype=np.float32)
        n = max(0, min(int(n), len(x)))
        fi, fo = got["f0_in"][i], got["f0_out"][i]
        kw = dict(J_max=got["J_max"], H_max=got["H_max"])
        if got["handed"] is not None:
            kw.update(marks=got["handed"][i][0], clamps=(got["handed"][i][1], got["K_max"]))
        ref = E.reference(x, n, fi, fo, geo, **kw)
        K, J = len(ref["marks"]), len(ref["syn"])
        if got["handed"] is None:
            assert got["n_marks"][i] == K, (i, got["n_marks"][i], K)
            diff = np.flatnonzero(got["marks"][i] != pad(ref["marks"], got["K_max"]))
            assert diff.size == 0, (i, "marks", diff[:4], got["marks"][i][diff[:4]], pad(ref["marks"], got["K_max"])[diff[:4]])
        assert got["n_syn"][i] == J, (i, got["n_syn"][i], J)
        assert np.array_equal(got["syn"][i], pad(ref["syn"], got["J_max"])) and np.array_equal(got["map"][i], pad(ref["map"], got["J_max"])), i
        want = np.zeros(L, dtype=np.float32)
        want[:len(x)] = ref["out"]
        wrong = bits(got["out"][i]) != bits(want)
        assert not wrong.any(), (i, int(wrong.sum()), np.flatnonzero(wrong)[:4])
        if fp64 and n > 0:
            r64 = E.reference(x, n, fi, fo, geo, dtype=np.float64, **kw)
            bound = R.fp32_bound(r64["den"], r64["grains"], float(np.abs(x[:n]).max()))
            safe = np.abs(r64["den"] - R.MIN_WEIGHT) > 1e-5              # (a weight sum on the floor may fall either way)
            err = np.abs(got["out"][i][:len(x)].astype(np.float64) - r64["out"])
            ratio = float((err[safe] / np.maximum(bound[safe], 1e-300)).max()) if safe.any() else 0.0
            worst = max(worst, ratio)
            print(f"{name or 'clip'} [{i}]: {K} marks, {J} synthesis marks, error / bound {ratio:.4f}")
            assert (err[safe] <= bound[safe]).all(), (i, float((err - bound)[safe].max()))
    if name and fp64:
        WORST[name] = max(WORST.get(name, 0.0), worst)
    return worst


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_kernels_equal_the_restatement(name):
    c = E.BY_NAME[name]
    x, fi, fo = E.build(c)
    clips = [(x, c.n, fi, fo)]
    got = launch(c.geo, clips)
    check(c.geo, clips, got, name=name)
    assert got["n_marks"][0] >= 20 and got["n_syn"][0] >= 20
    if name == "narrowest":
        assert got["K_max"] == got["J_max"] == got["L"] and got["n_marks"][0] > got["L"] // 4
    if name == "long":
        assert R.frame(int(got["marks"][0][got["n_marks"][0] - 1]), c.geo.hop, len(fi)) >= E.PS_FR


RAMPS = {"ring stress": (E.STRESS, None, 0), "seam frame": (E.STRESS, None, 2),"rising, P = 1024": (E.WIDE, 1024, 1), "falling, P = 1024": (E.WIDE, 1024, -1),
         "rising, defaults": (E.DEFAULT, 339, 1), "falling, defaults": (E.DEFAULT, 339, -1)}


@pytest.mark.parametrize("which", list(RAMPS))
def test_ramps_alone_and_as_a_row_among_nan_rows(which):
    geo, P, sign = RAMPS[which]
    if sign == 0:
        x, fi = E.stress()
        n = len(x)
        marks, searches = R.marks_trace(x, n, fi, geo.hop, geo.sr, geo.P_u, geo.P_min, geo.P_max, geo.alpha)
        w = E.ring_walk(marks, searches, geo.hop, len(fi))
        assert (w["step"], w["reach"]) == (2048, 2559) and w["advances"] >= 14             # (the host test's; cheap to restate)
    elif sign == 2:
        x, fi = E.seam()
        n = len(x)
        marks = R.marks_ref(x, n, fi, geo.hop, geo.sr, geo.P_u, geo.P_min, geo.P_max, geo.alpha)
        assert marks[4:6] == [E.PS_H, E.PS_H + 256]
    else:
        n = 60000
        x, fi = E.ramp(n, sign), E.constant_track(n, geo, P)
        marks = (E.rising_marks if sign > 0 else E.falling_marks)(n, P, geo.alpha)
    clips = [(x, n, fi, (fi * np.float32(0.8)).astype(np.float32))]
    alone = launch(geo, clips)
    assert alone["n_marks"][0] == len(marks) and np.array_equal(alone["marks"][0][:len(marks)], marks)
    check(geo, clips, alone, name=which)
    row = launch(geo, clips, rows=[2], B=3)
    for k in ("marks", "n_marks", "syn", "map", "n_syn"):
        assert np.array_equal(alone[k], row[k]), k
    assert np.array_equal(bits(alone["out"]), bits(row["out"]))


@pytest.mark.parametrize("L", [E.PS_TILE - 1, E.PS_TILE, E.PS_TILE + 1, 2 * E.PS_TILE + 1])
def test_rows_that_end_at_the_overlap_add_tile(L):
    c = E.SMALL
    x, fi, fo = E.build(c)
    T = 1 + L // c.geo.hop
    clips = [(x[:L], L, fi[:T], fo[:T]), (x[500:500 + L], L - 1, fi[:T], fo[:T])]
    got = launch(c.geo, clips, L=L)
    check(c.geo, clips, got, name=f"L = {L}")
    assert got["n_syn"].min() >= 5


def test_130_ragged_clips_each_as_if_alone():
    geo, B, L = E.DEFAULT, 130, 900
    rng = np.random.default_rng(5)
    lens = rng.integers(0, L + 1, B)
    lens[[0, 1, 63, 64, 127, 128, 129]] = [0, 1, L, 0, 1, L - 3, 517]
    T = 1 + L // geo.hop
    clips = []
    for b in range(B):
        f0 = (110.0, 150.0, 200.0, 310.0)[b % 4]
        fi = np.full(T, f0, dtype=np.float32)
        fi[rng.random(T) < 0.2] = 0.0
        ratio = (0.5, 0.8, 1.25, 2.0, 4.0)[b % 5]
        clips.append((E.harmonic(L, f0, geo.sr, seed=1000 + b), int(lens[b]), fi, (fi * np.float32(ratio)).astype(np.float32)))
    got = launch(geo, clips, L=L)
    check(geo, clips, got, name="130 clips")
    assert got["n_marks"][128] > 2 and got["n_marks"][129] > 2 and got["n_marks"][:2].tolist() == [0, 1]
    for b in range(B):
        one = launch(geo, clips[b:b + 1], L=L)
        for k in ("marks", "n_marks", "syn", "map", "n_syn"):
            assert np.array_equal(one[k][0], got[k][b]), (b, k)
        assert np.array_equal(bits(one["out"][0]), bits(got["out"][b])), b


def test_results_do_not_depend_on_the_buffers_sizes_or_the_launch():
    c = E.SMALL
    x, fi, fo = E.build(c)
    clips = [(x, c.n, fi, fo)]
    base = launch(c.geo, clips)
    check(c.geo, clips, base, name="small")
    again = launch(c.geo, clips)
    wide = launch(c.geo, clips, L=c.n + 1501, K_extra=37, J_extra=91)
    K, J = int(base["n_marks"][0]), int(base["n_syn"][0])
    assert K > 30 and J > 40 and wide["K_max"] > base["K_max"] + 37 and wide["J_max"] > base["J_max"] + 91
    for k in ("marks", "n_marks", "syn", "map", "n_syn"):
        assert np.array_equal(base[k], again[k]), k
        if k[0] != "n":
            w = base[k].shape[1]
            assert np.array_equal(wide[k][0][:w], base[k][0]) and (wide[k][0][w:] == -1).all(), k
    assert wide["n_marks"][0] == K and wide["n_syn"][0] == J
    assert np.array_equal(bits(base["out"]), bits(again["out"]))
    assert np.array_equal(bits(wide["out"][0][:c.n]), bits(base["out"][0])) and not bits(wide["out"][0][c.n:]).any()
    check(c.geo, clips, wide, fp64=False)


def test_lengths_null_and_outside_the_row():
    c = E.SMALL
    x, fi, fo = E.build(c)
    L = 3000
    T = 1 + L // c.geo.hop
    full = [(x[:L], L, fi[:T], fo[:T]), (x[L:2 * L], L, fi[:T], fo[:T])]
    own, null = launch(c.geo, full, L=L), launch(c.geo, full, L=L, lengths=None)
    check(c.geo, full, null, name="lengths NULL")
    for k in ("marks", "n_marks", "syn", "map", "n_syn", "out"):
        assert np.array_equal(own[k].view(np.int32), null[k].view(np.int32)), k
    clips = [(x[:L], 0, fi[:T], fo[:T]), (x[:L], L, fi[:T], fo[:T]), (x[:L], 1234, fi[:T], fo[:T])]
    got = launch(c.geo, clips, L=L, lengths=[-5, L + 1000, 1234])
    check(c.geo, clips, got, name="lengths outside")
    assert got["n_marks"].tolist()[0] == 0 and got["n_syn"][0] == 0 and not bits(got["out"][0]).any()
    assert np.array_equal(bits(got["out"][1]), bits(own["out"][0]))


def test_hostile_marks_and_counts_into_psola():
    c = E.SMALL
    x, fi, fo = E.build(c)
    true = launch(c.geo, [(x, c.n, fi, fo)])
    K, K_max = int(true["n_marks"][0]), true["K_max"]
    cases = E.hostile(true["marks"][0], K, K_max, c.n)
    assert len(cases) == 8
    clips = [(x, c.n, fi, fo)] * (len(cases) + 1)
    handed = list(cases.values()) + [(true["marks"][0], K)]
    got = launch(c.geo, clips, marks=handed)
    assert np.isfinite(got["out"]).all()
    check(c.geo, clips, got, fp64=False)
    assert np.array_equal(bits(got["out"][-1]), bits(true["out"][0])) and np.array_equal(got["syn"][-1], true["syn"][0])       # the true marks, handed in
    names = list(cases)
    for i, name in enumerate(names):
        J, n_cl = int(got["n_syn"][i]), len(R.clamped_marks(*handed[i], K_max, c.n))
        assert (got["syn"][i][:J] >= 0).all() and (got["syn"][i][:J] < c.n).all() and (got["map"][i][:J] >= 0).all() and (got["map"][i][:J] < max(n_cl, 1)).all(), name
        if name in ("count -5", "count 0"):
            assert J == 0 and np.array_equal(bits(got["out"][i]), bits(x)), name                                  # no mark: the input
        else:
            assert J >= 1 and not np.array_equal(bits(got["out"][i]), bits(true["out"][0])), name
    gaps = np.diff(R.clamped_marks(*handed[names.index("2^31 - 1")], K_max, c.n))
    assert gaps.max() > true["H_max"]                                    # marks further apart than H_max: the walk over s_j cuts the grain


def test_ratio_edges_clamps_and_exact_ties():
    geo, n = E.DEFAULT, E.EDGE_N
    x = E.pulses(n, 147)
    fi, fo = E.edge_tracks(n, geo)
    clips = [(x, n, fi, fo)]
    got = launch(geo, clips)
    check(geo, clips, got, name="ratio edges")
    K, J = int(got["n_marks"][0]), int(got["n_syn"][0])
    assert K == 41 and (np.diff(got["marks"][0][:K]) == 147).all()
    s = got["syn"][0][:J]
    edge = (np.array([R.frame(int(v), geo.hop, len(fi)) for v in s[:-1]]) // 3) % len(E.RATIO_EDGES)
    step = np.diff(s)
    for e, want in enumerate((588, 37, 588, 37, 588, 37, 221, 74)):       # 147 / r: 0.25, 4, below, above, just inside twice, the two ties up
        assert (edge == e).any() and (step[edge == e] == want).all(), (e, want, step[edge == e])
