"""GPU: nsg_audio_resample and nsg_audio_trim_bounds against the fp64 statements of their formulas (tests/helpers/
resample64.py) with bounds derived from those formulas, the batch-independence both promise, and the CMU Arctic writer built on
them.  parity unpinned: librosa and resampy are absent, and the reference holds no waveform."""
import functools
import os

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import audio as Au, data as Dm, preprocess as P
from tests.helpers import resample64 as R

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

TILE = 256                                                       # csrc/resample.hip RS_TILE: outputs per workgroup
RATES = [(16000, 22050), (48000, 22050), (44100, 22050), (11025, 22050), (22050, 16000)]


def lengths_for(sr_in, sr_out):
    """50 (shorter than the filter's half width), 3001, and the two input lengths whose outputs end either side of the first
    tile boundary: ceil(a P / Q) <= 256 < ceil((a + 1) P / Q)."""
    p, q = R.ratio(sr_in, sr_out)
    a = TILE * q // p
    assert -(-a * p // q) <= TILE < -(-(a + 1) * p // q)
    return [50, 3001, a, a + 1]


@functools.lru_cache(maxsize=None)
def noise_case(sr_in, sr_out, L):
    """(x float32, y64, A): uniform noise in [-1, 1) and its fp64 resampling, computed once per (rates, length)."""
    x = np.random.RandomState(L).uniform(-1, 1, L).astype(np.float32)
    y, A = R.resample64(x, sr_in, sr_out)
    for a in (y, A):
        a.setflags(write=False)
    return x, y, A


def bound(sr_in, sr_out, A):
    """One rounding per coefficient and one per fmaf of the 2W-term chain, each at most 2^-24 of the sum of the terms'
    magnitudes (first order)."""
    p, q = R.ratio(sr_in, sr_out)
    return (2 * R.half_width(p, q) + 2) * 2.0 ** -24 * A + 1e-12


@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_resample_matches_the_fp64_formula(sr_in, sr_out):
    p, q = R.ratio(sr_in, sr_out)
    worst = err = 0.0
    for L in lengths_for(sr_in, sr_out):
        x, y64, A = noise_case(sr_in, sr_out, L)
        y = Au.resample(x, sr_in, sr_out)
        assert y.dtype == np.float32 and y.shape == y64.shape == (-(-L * p // q),)
        e = np.abs(y.astype(np.float64) - y64)
        b = bound(sr_in, sr_out, A)
        worst, err = max(worst, float((e / b).max())), max(err, float(e.max()))
        print(f"{sr_in} -> {sr_out}, {L} samples: max |y - y64| = {e.max():.3e}, max error / bound = {(e / b).max():.3e}, max A = {A.max():.3f}")
        assert (e <= b).all(), (sr_in, sr_out, L, float((e / b).max()))
    print(f"{sr_in} -> {sr_out}: largest error {err:.3e}, largest error / bound {worst:.3e}")


@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_resampled_sine_is_the_sine_at_the_new_rate(sr_in, sr_out):
    """Independent of the helper's sum: a sine inside the pass band comes out as the same sine sampled at the new rate, away
    from the ends (the fp64 formula itself is within 7.8e-8 of it for these rates)."""
    p, q = R.ratio(sr_in, sr_out)
    W = R.half_width(p, q)
    cut = int(2 * W * max(1.0, p / q)) + 8
    L = 6000
    for f in (1000.0, 0.45 * R.ROLLOFF * min(sr_in, sr_out)):
        x = np.sin(2 * np.pi * f * np.arange(L) / sr_in).astype(np.float32)
        y = Au.resample(x, sr_in, sr_out).astype(np.float64)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / sr_out)
        _, A = R.resample64(x, sr_in, sr_out)
        e = np.abs(y - want)[cut:-cut]
        b = (bound(sr_in, sr_out, A) + 1e-7)[cut:-cut]
        assert len(e) > 1000
        print(f"{sr_in} -> {sr_out}, {f:.1f} Hz: max |y - sine| = {e.max():.3e}, max error / bound = {(e / b).max():.3e}")
        assert (e <= b).all(), (sr_in, sr_out, f, float((e / b).max()))


@pytest.mark.parametrize("sr_in,sr_out", [(16000, 22050), (48000, 22050)])
def test_ragged_resample_equals_each_clip_alone(sr_in, sr_out):
    p, q = R.ratio(sr_in, sr_out)
    lens = lengths_for(sr_in, sr_out) + [1777]                    # the shortest and the longest among them
    clips = [noise_case(sr_in, sr_out, L)[0] for L in lens]
    alone = [Au.resample(c, sr_in, sr_out) for c in clips]
    for order in (range(5), (1, 4, 0, 3, 2)):
        batch = np.zeros((5, max(lens) + 37), dtype=np.float32)   # wider than the longest clip: L_in is not the clip's length
        for r, i in enumerate(order):
            batch[r, :lens[i]] = clips[i]
        out, out_lens = Au.resample(torch.from_numpy(batch).to(DEV), sr_in, sr_out, lengths=[lens[i] for i in order])
        assert out.is_cuda and tuple(out.shape) == (5, -(-batch.shape[1] * p // q))
        assert out_lens.dtype == np.int32 and out_lens.tolist() == [-(-lens[i] * p // q) for i in order]
        out = out.cpu().numpy()
        for r, i in enumerate(order):
            assert np.array_equal(out[r, :out_lens[r]], alone[i]), (order, r)
            assert not out[r, out_lens[r]:].any()
    # without lengths every row is L_in samples long; the numpy form is the tensor form of one row
    full, full_lens = Au.resample(torch.from_numpy(batch).to(DEV), sr_in, sr_out)
    assert full_lens.tolist() == [full.shape[1]] * 5
    assert np.array_equal(full[2].cpu().numpy(), Au.resample(batch[2], sr_in, sr_out))


TRIM_CASES = [(16000, 4000, 11000, (3072, 12288)), (9000, 0, 5200, (0, 6656)), (5000, 2100, 5000, (1536, 5000)),
              (1025, 0, 1025, (0, 1025)), (20480, 7000, 9000, (6144, 10240))]


@functools.lru_cache(maxsize=None)
def trim_clips():
    """1e-3 noise, plus a 0.5-amplitude 220 Hz tone with 0.1 noise over [a, b): seed-7 draws, in TRIM_CASES' order."""
    rs = np.random.RandomState(7)
    clips = []
    for L, a, b, _ in TRIM_CASES:
        y = 1e-3 * rs.randn(L)
        y[a:b] += 0.5 * np.sin(2 * np.pi * 220 * np.arange(a, b) / 22050) + 0.1 * rs.randn(b - a)
        clips.append(y.astype(np.float32))
    return clips


@pytest.mark.parametrize("frame_length,hop", [(2048, 512), (512, 128), (64, 8)])
def test_trim_bounds_are_the_fp64_formulas(frame_length, hop):
    """Exact equality with trim64, asserted only after the condition that makes it derivable: every frame is at least 0.01 dB
    from the threshold, and fp32 summation of a frame of <= 2048 squares moves its level by at most
    10 log10(1 + 2 * 2050 * 2^-24) = 1.1e-3 dB.  The bounds kernel takes 256 frames a round, a wave 64 of them: at (2048, 512)
    every clip has fewer than 64 frames (3 .. 41: whole waves own none), at (64, 8) four of the five more than 256 (129 .. 2561)."""
    clips = trim_clips()
    want = []
    for y, (_, _, _, table) in zip(clips, TRIM_CASES):
        b64, margin = R.trim64(y, 20.0, frame_length, hop)
        assert margin >= 0.01, (len(y), margin)
        if (frame_length, hop) == (2048, 512):
            assert b64 == table
        want.append(b64)
    lens = [len(y) for y in clips]
    batch = np.zeros((len(clips), max(lens) + 100), dtype=np.float32)
    for r, y in enumerate(clips):
        batch[r, :lens[r]] = y
    got = Au.trim_silence(torch.from_numpy(batch).to(DEV), 20.0, frame_length, hop, lengths=lens)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (len(clips), 2)
    assert [tuple(r) for r in got.cpu().tolist()] == want
    for y, b64 in zip(clips, want):                               # each clip alone, in the numpy form: librosa's return value
        trimmed, (start, end) = Au.trim_silence(y, 20.0, frame_length, hop)
        assert (start, end) == b64 and np.array_equal(trimmed, y[start:end]) and trimmed.dtype == np.float32
    # without lengths a row is L samples long: the zero padding is part of the clip
    b64, margin = R.trim64(batch[0], 20.0, frame_length, hop)
    assert margin >= 0.01
    assert tuple(Au.trim_silence(torch.from_numpy(batch[:1]).to(DEV), 20.0, frame_length, hop).cpu().tolist()[0]) == b64


def _cmu_arctic_tree(root, speakers=("awb", "bdl"), seed=0):
    """2 speakers x 2 int16 wavs at 16 kHz of about 0.6 s: a tone burst with a little noise between silent ends."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    paths = []
    for spk in speakers:
        d = os.path.join(root, "cmu_us_%s_arctic" % spk, "wav")
        os.makedirs(d)
        for name in ("arctic_a0002", "arctic_a0001"):             # written out of order: the walker sorts
            L = int(rs.uniform(0.55, 0.65) * 16000)
            a, b = int(rs.uniform(0.15, 0.25) * L), int(rs.uniform(0.75, 0.85) * L)
            y = 1e-3 * rs.randn(L)
            y[a:b] += rs.uniform(0.3, 0.6) * np.sin(2 * np.pi * rs.uniform(150, 400) * np.arange(a, b) / 16000) + 0.05 * rs.randn(b - a)
            wavfile.write(os.path.join(d, name + ".wav"), 16000, (y / np.abs(y).max() * 0.8 * 32767).astype(np.int16))
        paths += [os.path.join(d, n + ".wav") for n in ("arctic_a0001", "arctic_a0002")]
    return paths


def test_cmu_arctic_writer(tmp_path):
    src = str(tmp_path / "cmu_arctic")
    paths = _cmu_arctic_tree(src)
    outs = {}
    for bc in (1, 64):
        outs[bc] = str(tmp_path / ("out%d" % bc))
        meta = P.build_from_path_cmu_arctic(src, outs[bc], speakers=("awb", "bdl"), batch_clips=bc)
    root = outs[64]
    names = sorted(os.listdir(root))
    assert names == sorted(["train.txt"] + ["cmu_arctic-%s-%05d.npy" % (k, i) for k in ("audio", "mel") for i in range(1, 5)])
    assert sorted(os.listdir(outs[1])) == names
    for nm in names:
        assert open(os.path.join(outs[1], nm), "rb").read() == open(os.path.join(root, nm), "rb").read(), nm
    rows = [ln.split("|") for ln in open(os.path.join(root, "train.txt"), encoding="utf-8").read().splitlines()]
    assert [tuple(r[:2]) + (int(r[2]), r[3], int(r[4])) for r in rows] == [tuple(m) for m in meta]
    assert [int(r[4]) for r in rows] == [0, 0, 1, 1]
    for i, (r, path) in enumerate(zip(rows, paths), start=1):
        assert r[0] == "cmu_arctic-audio-%05d.npy" % i and r[1] == "cmu_arctic-mel-%05d.npy" % i and r[3] == "N/A"
        # the composition of the public functions on this clip alone, in cmu_arctic.py's order: load + resample, trim, rescale, mel
        wav = Au.load_wav(path, 22050, resample=True)
        sr, native = Au.read_wav(path)
        assert sr == 16000 and len(wav) == -(-len(native) * 441 // 320)
        wav, (start, end) = Au.trim_silence(wav, 20.0)
        assert 0 < start < end < -(-len(native) * 441 // 320) and end - start > 0.5 * len(native)    # both silent ends are cut
        wav = (wav / float(np.abs(wav).max()) * 0.999).astype(np.float32)
        N = 1 + len(wav) // 256
        mel = np.load(os.path.join(root, r[1]), allow_pickle=False)
        assert mel.dtype == np.float32 and mel.shape == (N, 80)
        assert np.array_equal(mel, Au.melspectrogram(wav).T)
        audio = np.load(os.path.join(root, r[0]), allow_pickle=False)
        left, right = P.lws_pad_lr(wav, 1024, 256)
        assert audio.dtype == np.float32 and int(r[2]) == N * 256
        assert np.array_equal(audio, np.pad(wav, (left, right))[:N * 256])
    # the reader: every utterance comes back once over the two splits, with its speaker id
    seen = {}
    for train in (True, False):
        ds = Dm.MelSpecDataSource(root, train=train)
        assert ds.multi_speaker
        seen.update({os.path.basename(pth): g for pth, g in zip(ds.paths, ds.speaker_ids)})
    assert seen == {"cmu_arctic-mel-%05d.npy" % i: (i - 1) // 2 for i in range(1, 5)}
    loaders = Dm.get_data_loaders(root, batch_size=4, max_time_steps=32 * Dm.HOP_SIZE, num_workers=0, with_audio=True)
    ids = []
    for phase in ("train", "test"):
        for x, y, c, g, lens in loaders[phase]:
            assert c.shape[1] == 80 and x.shape[2] == c.shape[2] * 256 and g.dtype == torch.int64
            ids += g.tolist()
    assert sorted(ids) == [0, 0, 1, 1]
    # the defaults are the LJSpeech path's: a file at another rate is still refused
    with pytest.raises(ValueError, match="16000"):
        P.process_utterances(paths, ["N/A"] * 4, str(tmp_path / "refused"), "cmu_arctic", 1, [0, 0, 1, 1])
