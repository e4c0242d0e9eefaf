"""GPU: nsg_audio_pitch_marks and nsg_audio_psola equal the restatement of their contract (tests/helpers/psola_ref.py) bit for
bit -- marks, counts, synthesis marks, mapping, and the samples against the fp32 statement -- and are close to the fp64 statement
within the bound the helper derives from the roundings; the identity; independence of the batch; hostile tracks; and what the
operator is for: the pitch moves, the spectral envelope stays where audio.pitch_shift moves it.  Every output buffer is filled
with 0xFF before the launch and compared whole, so every comparison also shows that each element was written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio, ops  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import psola_ref as R  # noqa: E402

DEV = "cuda:0"
SR, HOP = 22050, 256
P_U, P_MIN, P_MAX = 110, 45, 339
RATIOS = (0.5, 0.8, 1.0, 1.25, 2.0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def launch(clips, L=None, rows=None):
    """Both entry points on the clips [(x, n, f0_in, f0_out)], clip i in row rows[i] of a batch of max(rows) + 1 rows of L samples
    (NaN past each clip's n, NaN rows elsewhere), every output poisoned -> dict of numpy arrays."""
    rows = list(range(len(clips))) if rows is None else rows
    B = max(rows) + 1
    L = max(1, max(len(c[0]) for c in clips)) if L is None else L
    T = 1 + L // HOP
    wav = np.full((B, L), np.nan, dtype=np.float32)
    lens = np.zeros(B, dtype=np.int32)
    fi, fo = np.zeros((B, T), dtype=np.float32), np.zeros((B, T), dtype=np.float32)
    for r, (x, n, a, b) in zip(rows, clips):
        a, b = a[:T], b[:T]
        wav[r, :n] = x[:n]
        lens[r] = n
        fi[r, :len(a)], fo[r, :len(b)] = a, b
        fi[r, len(a):], fo[r, len(b):] = (a[-1], b[-1]) if len(a) else (0, 0)          # frames past the clip's own track: its last
    _, K_max, _, _, J_max = R.sizes(L, P_MIN, P_MAX)
    d = lambda a: torch.from_numpy(a).to(DEV)
    poison = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=DEV)          # 0xFFFFFFFF: a NaN where floats are written
    wav_d, lens_d, fi_d, fo_d = d(wav), d(lens), d(fi), d(fo)
    marks, n_marks, syn, mp, n_syn, out = poison(B, K_max), poison(B), poison(B, J_max), poison(B, J_max), poison(B), poison(B, L)
    marks.fill_(-2); syn.fill_(-2); mp.fill_(-2)                          # (-1 is a value the kernels write)
    consts = (B, L, T, HOP, float(SR), P_U, P_MIN, P_MAX, 1, 4, K_max)
    _lib.call("nsg_audio_pitch_marks", _p(wav_d), _p(lens_d), _p(fi_d), _p(marks), _p(n_marks), *consts, _stream())
    _lib.call("nsg_audio_psola", _p(wav_d), _p(lens_d), _p(fi_d), _p(fo_d), _p(marks), _p(n_marks), _p(syn), _p(mp), _p(n_syn), _p(out), *consts,
              J_max, _stream())
    res = dict(marks=marks, n_marks=n_marks, syn=syn, map=mp, n_syn=n_syn, out=out.view(torch.float32))
    return {k: v.cpu().numpy()[rows] for k, v in res.items()}, (fi[rows], fo[rows])


def check(clips, got, tracks, fp64=True):
    """Row i of `got` against the restatement of clip i, whole rows: the -1 and +0.0 padding included."""
    for i, (x, n, _, _) in enumerate(clips):
        x = x[:got["out"].shape[1]]
        fi, fo = tracks[0][i], tracks[1][i]
        ref = R.psola_ref(x, n, fi, fo, HOP, SR, P_U, P_MIN, P_MAX)
        K, J = len(ref["marks"]), len(ref["syn"])
        assert got["n_marks"][i] == K and got["n_syn"][i] == J, (i, got["n_marks"][i], K, got["n_syn"][i], J)
        pad = lambda v, m: np.concatenate([np.asarray(v, dtype=np.int32), np.full(m - len(v), -1, dtype=np.int32)])
        assert np.array_equal(got["marks"][i], pad(ref["marks"], got["marks"].shape[1])), i
        assert np.array_equal(got["syn"][i], pad(ref["syn"], got["syn"].shape[1])) and np.array_equal(got["map"][i], pad(ref["map"], got["map"].shape[1])), i
        L = got["out"].shape[1]
        want = np.zeros(L, dtype=np.float32)
        want[:len(x)] = ref["out"]
        assert np.array_equal(bits(got["out"][i]), bits(want)), (i, int((bits(got["out"][i]) != bits(want)).sum()))
        if fp64 and n > 0:
            r64 = R.psola_ref(x, n, fi, fo, HOP, SR, P_U, P_MIN, P_MAX, dtype=np.float64)
            bound = R.fp32_bound(r64["den"], r64["grains"], float(np.abs(x[:n]).max()))
            safe = np.abs(r64["den"] - R.MIN_WEIGHT) > 1e-5              # (a weight sum on the floor may fall either way)
            err = np.abs(got["out"][i][:len(x)].astype(np.float64) - r64["out"])
            assert (err[safe] <= bound[safe]).all(), (i, float((err - bound)[safe].max()))


@pytest.fixture(scope="module")
def vowels():
    """Four steady vowels of 0.3 s (three halves of the marks kernel's ring) and their ideal tracks."""
    out = []
    for k, f in enumerate((80.0, 110.0, 180.0, 400.0)):
        x, voiced = R.vowel(f, 0.3, formant=900.0 + 150.0 * k, seed=k)
        out.append((x, R.track(voiced, f, HOP)))
    return out


@pytest.mark.parametrize("ratio", RATIOS)
def test_constant_f0_at_every_ratio(vowels, ratio):
    clips = [(x, len(x), f, (f * np.float32(ratio)).astype(np.float32)) for x, f in vowels]
    got, tracks = launch(clips)
    check(clips, got, tracks)
    assert (got["n_marks"] >= [22, 31, 52, 115]).all()
    if ratio != 1.0:
        assert (np.abs(got["n_syn"] / got["n_marks"] - ratio) < 0.15 * ratio).all()


def test_glide_voicing_switches_and_a_per_frame_target():
    n = int(0.6 * SR)
    glide = np.linspace(100.0, 200.0, n)
    x0, v0 = R.vowel(glide, 0.6)
    f0 = R.track(v0, glide, HOP)
    x1, v1 = R.vowel(140.0, 0.6, unvoiced=((0.2, 0.35),), seed=3)
    f1 = R.track(v1, 140.0, HOP)
    t = np.arange(len(f1))
    wobble = (150.0 * 2.0 ** (0.3 * np.sin(t / 5.0))).astype(np.float32)       # a per-frame target, voiced where the source is not too
    clips = [(x0, n, f0, np.full_like(f0, 150.0)), (x1, n, f1, (f1 * np.float32(1.25)).astype(np.float32)), (x1, n, f1, wobble),
             (x0, n - 777, f0, (f0 * np.float32(0.8)).astype(np.float32))]           # the last range is cut by the clip's end
    got, tracks = launch(clips)
    check(clips, got, tracks)
    gaps = np.diff(got["marks"][1][:got["n_marks"][1]])
    assert (gaps == P_U).sum() >= 25 and ((gaps > 150) & (gaps < 165)).sum() >= 40          # 5 ms marks in the noise, the period outside


def test_edges_ties_and_short_clips():
    flat = np.zeros(3000, dtype=np.float32)
    flat[100:104] = 1.0                                                   # flat-topped pulses: the smallest index of the maximum
    flat[300:303] = 1.0
    flat[495:505] = -0.0                                                  # and a range of zeros of both signs: +0.0 is the greater
    f = np.full(1 + 3000 // HOP, 110.0, dtype=np.float32)
    up = (f * np.float32(1.25)).astype(np.float32)
    x, _ = R.vowel(110.0, 0.3)
    clips = [(flat, 3000, f, up), (x, 150, f, up), (x, 0, f, up), (x, 1, f, up)]
    got, tracks = launch(clips, L=3000)
    check(clips, got, tracks)
    assert got["marks"][0][0] == 100 and got["marks"][0][1] == 300
    assert got["n_marks"].tolist()[1:] == [1, 0, 1] and got["n_syn"].tolist()[1:] == [1, 0, 1]
    assert np.array_equal(bits(got["out"][1][:150]), bits(x[:150])) and not got["out"][2].any()
    one, tr = launch([(x, 1, f[:1], up[:1])], L=1)                         # a batch whose rows are one sample long
    check([(x[:1], 1, f[:1], up[:1])], one, tr)


def test_identity_returns_the_input(vowels):
    x, f = vowels[1]
    x2, v2 = R.vowel(140.0, 0.3, unvoiced=((0.1, 0.2),), seed=3)
    f2 = R.track(v2, 140.0, HOP)
    clips = [(x, len(x), f, f), (x, len(x), np.zeros_like(f), np.full_like(f, 200.0)), (x2, len(x2), f2, f2)]        # ratio 1; all unvoiced; mixed
    got, tracks = launch(clips)
    check(clips, got, tracks)
    for i, (x, n, _, _) in enumerate(clips):
        K = got["n_marks"][i]
        marks = got["marks"][i][:K]
        assert got["n_syn"][i] == K and np.array_equal(got["syn"][i][:K], marks) and np.array_equal(got["map"][i][:K], np.arange(K))
        m0, m1 = marks[0], marks[-1]
        out = got["out"][i]
        assert np.array_equal(bits(out[:m0 + 1]), bits(x[:m0 + 1])) and np.array_equal(bits(out[m1:n]), bits(x[m1:n]))      # outside: exactly
        assert np.array_equal(bits(out[marks]), bits(x[marks]))
        r64 = R.psola_ref(x, n, tracks[0][i], tracks[1][i], HOP, SR, P_U, P_MIN, P_MAX, dtype=np.float64)
        bound = R.fp32_bound(r64["den"], r64["grains"], float(np.abs(x).max()))
        assert (np.abs(out[:n].astype(np.float64) - x) <= bound).all() and bound.max() < 1e-5                               # between: the roundings


def test_a_clip_alone_and_in_a_batch_give_the_same_bits(vowels):
    x, f = vowels[2]
    n = len(x) - 313
    up = (f * np.float32(1.25)).astype(np.float32)
    alone, _ = launch([(x, n, f, up)], L=n)
    y, fy = vowels[0]
    both, _ = launch([(y, len(y), fy, fy), (x, n, f, up)], L=len(x) + 1501, rows=[0, 2])
    K, J = alone["n_marks"][0], alone["n_syn"][0]
    assert both["n_marks"][1] == K and both["n_syn"][1] == J and K > 40 and J > 50
    assert np.array_equal(alone["marks"][0][:K], both["marks"][1][:K]) and (both["marks"][1][K:] == -1).all()
    assert np.array_equal(alone["syn"][0][:J], both["syn"][1][:J]) and np.array_equal(alone["map"][0][:J], both["map"][1][:J])
    assert np.array_equal(bits(alone["out"][0][:n]), bits(both["out"][1][:n])) and not both["out"][1][n:].any()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, -100.0, 1e-30, 1e30])
def test_hostile_tracks_stay_inside_the_clip(vowels, value):
    x, f = vowels[1]
    bad = np.full_like(f, value)
    mixed = f.copy()
    mixed[::3] = value
    clips = [(x, len(x), bad, f), (x, len(x), f, bad), (x, len(x), mixed, (f * np.float32(2.0)).astype(np.float32)), (x, len(x) - 100, bad, bad)]
    got, tracks = launch(clips)
    check(clips, got, tracks, fp64=False)
    for i, (x, n, _, _) in enumerate(clips):
        K, J = got["n_marks"][i], got["n_syn"][i]
        assert K >= 1 and (got["marks"][i][:K] >= 0).all() and (got["marks"][i][:K] < n).all() and (np.diff(got["marks"][i][:K]) > 0).all()
        assert J >= 1 and (got["syn"][i][:J] >= 0).all() and (got["syn"][i][:J] < n).all() and (got["map"][i][:J] < K).all()
        assert np.isfinite(got["out"][i]).all()


def test_the_wrappers_give_the_entry_points_results(vowels):
    clips = [(x, len(x), f, (f * np.float32(r)).astype(np.float32)) for (x, f), r in zip(vowels, (0.8, 1.25, 1.0, 2.0))]
    want, _ = launch(clips)
    wav = torch.from_numpy(np.stack([c[0] for c in clips])).to(DEV)
    f0 = torch.from_numpy(np.stack([c[2] for c in clips])).to(DEV)
    out, marks, n_marks, syn, mp, n_syn = audio.pitch_shift_psola(wav, f0, ratio=[0.8, 1.25, 1.0, 2.0], detail=True)
    for k, v in dict(out=out, marks=marks, n_marks=n_marks, syn=syn, map=mp, n_syn=n_syn).items():
        assert np.array_equal(v.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    m2, n2 = audio.pitch_marks(wav, f0)
    assert torch.equal(m2, marks) and torch.equal(n2, n_marks)
    tgt = torch.from_numpy(np.stack([c[3] for c in clips])).to(DEV)
    assert torch.equal(audio.pitch_shift_psola(wav, f0, target_f0=tgt), out)
    x, f = vowels[1]                                                      # numpy in, numpy out
    y, mk, K, s, a, J = audio.pitch_shift_psola(x, f, ratio=1.25, detail=True)
    assert np.array_equal(bits(y), bits(want["out"][1])) and K == want["n_marks"][1] and np.array_equal(mk, want["marks"][1][:K])
    assert J == want["n_syn"][1] and np.array_equal(s, want["syn"][1][:J]) and np.array_equal(a, want["map"][1][:J])
    mk2, K2 = audio.pitch_marks(x, f)
    assert K2 == K and np.array_equal(mk2, mk)
    lens = np.array([len(x) - 500, 300, 0, len(x)])
    cut = audio.pitch_shift_psola(wav, f0, ratio=1.25, lengths=lens)
    assert all(not cut[b, n:].any() for b, n in enumerate(lens)) and torch.equal(cut[3], audio.pitch_shift_psola(wav[3:], f0[3:], ratio=1.25)[0])


def test_perturb_pitch_draws_one_shift_per_clip(vowels):
    wav = torch.from_numpy(np.stack([v[0] for v in vowels])).to(DEV)
    a, pa = audio.perturb_pitch(wav, None, torch.Generator().manual_seed(3))
    b, pb = audio.perturb_pitch(wav, None, torch.Generator().manual_seed(3))
    c, pc = audio.perturb_pitch(wav, None, torch.Generator().manual_seed(4), tracker="viterbi")
    assert torch.equal(a, b) and np.array_equal(pa["ratio"], pb["ratio"]) and not torch.equal(a, c) and a.shape == wav.shape
    assert np.array_equal(pa["ratio"], audio.pitch_draws(4, torch.Generator().manual_seed(3))["ratio"])
    f0, _ = audio.f0(wav)
    assert torch.equal(pa["f0"], f0) and torch.equal(a, audio.pitch_shift_psola(wav, f0, ratio=pa["ratio"]))


@pytest.mark.parametrize("ratio,num,den", [(0.8, 4, 5), (1.25, 5, 4)])
def test_the_pitch_moves_and_the_envelope_stays(ratio, num, den):
    """The synthetic vowel at 110 Hz under a 1 kHz resonance.  (A CPU prototype of the definition gave F0 87.8 and 137.8 Hz with
    the strongest harmonic at 966 and 964 Hz, where plain resampling put it at 791 and 1 238 Hz.)"""
    x, _ = R.vowel(110.0, 0.6)
    f, _ = audio.f0(x)
    y = audio.pitch_shift_psola(x, f, ratio=ratio)
    assert y.shape == x.shape and y.dtype == np.float32
    fy, _ = audio.f0(y)
    med = float(np.median(fy[fy > 0]))
    lag = SR / (110.0 * ratio)
    print(f"ratio {ratio}: median F0 {med:.2f} Hz for {110.0 * ratio:.2f} Hz")
    assert SR / (lag + 1.0) <= med <= SR / (lag - 1.0)                     # within one lag step
    z = audio.pitch_shift(x, num, den)
    mel = lambda w: audio.melspectrogram(torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))[None].to(DEV))
    ours, _ = audio.mel_cepstral_distortion(mel(y), mel(x))
    theirs, _ = audio.mel_cepstral_distortion(mel(z), mel(x))
    print(f"ratio {ratio}: MCD against the input {float(ours):.3f} dB by PSOLA, {float(theirs):.3f} dB by tempo + resample")
    assert float(ours) < float(theirs)
