"""The preprocessing writer (preprocess.py) that data.py is the reader of, load_wav, and the argument checks of
audio.melspectrogram and its C entry point.  CPU tests are unmarked (no kernel is launched); the ones that run the kernel are
marked gpu."""
import ctypes
import os

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio as Au, data as Dm, preprocess as P
from tests.helpers import mel_forward64 as H

DEV = "cuda:0"
gpu = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_lws_helpers_are_the_references_formulas():
    fsize, hop = 1024, 256
    for n in [hop * k + d for k in (1, 3, 40, 391) for d in (-1, 0, 1)] + [513, 100000]:
        pad = fsize - hop                                        # audio_tacotron.py:122-140, written out once more
        M = (n + 2 * pad - fsize) // hop + (1 if n % hop == 0 else 2)
        assert P.lws_num_frames(n, fsize, hop) == M
        left, right = P.lws_pad_lr(np.zeros(n), fsize, hop)
        assert (left, right) == (pad, pad + (M - 1) * hop + fsize - (n + 2 * pad))
        assert right >= pad and (n + left + right - fsize) % hop == 0
        assert n + left + right >= (1 + n // hop) * hop          # the cut to N * hop never runs past the padded audio


@pytest.mark.parametrize("speakers", [None, [3, 0, 3, 1, 0, 2, 2, 1, 0, 3, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3]])
def test_write_metadata_is_what_the_data_sources_read(tmp_path, speakers):
    n = 20
    root = str(tmp_path)
    meta = []
    for i in range(n):
        row = ("x-audio-%05d.npy" % (i + 1), "x-mel-%05d.npy" % (i + 1), 256 * (10 + i), "text %d, with a comma" % i)
        meta.append(row + (speakers[i],) if speakers else row)
    P.write_metadata(meta, root)
    lines = open(os.path.join(root, "train.txt"), encoding="utf-8").read().splitlines()
    assert lines == ["|".join(str(x) for x in m) for m in meta]
    seen = set()
    for train in (True, False):
        mel, wav = Dm.MelSpecDataSource(root, train=train), Dm.RawAudioDataSource(root, train=train)
        assert mel.multi_speaker == (speakers is not None) and len(mel) == len(wav) == (19 if train else 1)
        for k, (pm, pw) in enumerate(zip(mel.paths, wav.paths)):
            i = int(os.path.basename(pm)[6:11]) - 1
            seen.add(i)
            assert pm == os.path.join(root, meta[i][1]) and pw == os.path.join(root, meta[i][0])
            assert mel.lengths[k] == wav.lengths[k] == meta[i][2]
            if speakers:
                assert mel.speaker_ids[k] == speakers[i]
    assert seen == set(range(n))


def test_load_wav_formats_and_rate(tmp_path):
    from scipy.io import wavfile
    rs = np.random.RandomState(0)
    x16 = rs.randint(-32768, 32768, 3000).astype(np.int16)
    x16[:2] = (-32768, 32767)
    wavfile.write(str(tmp_path / "a.wav"), 22050, x16)
    a = Au.load_wav(str(tmp_path / "a.wav"))
    assert a.dtype == np.float32 and a.shape == (3000,) and np.array_equal(a, x16.astype(np.float32) / 32768.0)
    assert a.min() == -1.0 and a.max() < 1.0
    xf = rs.uniform(-1, 1, 2000).astype(np.float32)
    wavfile.write(str(tmp_path / "f.wav"), 22050, xf)
    assert np.array_equal(Au.load_wav(str(tmp_path / "f.wav")), xf)
    st = np.stack([x16, -x16 // 2], axis=1)
    wavfile.write(str(tmp_path / "s.wav"), 22050, st)
    assert np.array_equal(Au.load_wav(str(tmp_path / "s.wav")), a)                    # the first channel
    x32 = (x16.astype(np.int32) << 16)
    wavfile.write(str(tmp_path / "i.wav"), 22050, x32)
    assert np.array_equal(Au.load_wav(str(tmp_path / "i.wav")), a)
    x8 = rs.randint(0, 256, 1000).astype(np.uint8)
    wavfile.write(str(tmp_path / "u.wav"), 22050, x8)
    assert np.array_equal(Au.load_wav(str(tmp_path / "u.wav")), (x8.astype(np.float32) - 128) / 128)
    wavfile.write(str(tmp_path / "r.wav"), 16000, x16)
    with pytest.raises(ValueError, match="16000"):
        Au.load_wav(str(tmp_path / "r.wav"))
    assert Au.load_wav(str(tmp_path / "r.wav"), 16000).shape == (3000,)


def test_melspectrogram_checks_its_arguments_before_any_launch():
    """Every refusal below happens before the device is touched: this runs without a GPU."""
    y = np.zeros(4096, dtype=np.float32)
    with pytest.raises(TypeError):
        Au.melspectrogram(y.astype(np.int16))
    with pytest.raises(TypeError):
        Au.melspectrogram(np.zeros((2, 4096), dtype=np.float32))                     # numpy batches are not a form of the call
    with pytest.raises(TypeError):
        Au.melspectrogram(torch.zeros(2, 4096, dtype=torch.float64))
    with pytest.raises(TypeError):
        Au.melspectrogram(torch.zeros(4096))
    with pytest.raises(ValueError, match="layout"):
        Au.melspectrogram(y, layout="time_major")
    with pytest.raises(ValueError, match="fft_size"):
        Au.melspectrogram(y, fft_size=1000)
    with pytest.raises(ValueError, match="hop_size"):
        Au.melspectrogram(y, hop_size=0)
    with pytest.raises(ValueError, match="reflect"):
        Au.melspectrogram(np.zeros(512, dtype=np.float32))
    w = torch.zeros(3, 4096)
    for bad in ([4096, 4097, 4096], [4096, 512, 4096], [4096, 4096], [[4096, 4096, 4096]], [4096.0, 4096.0, 4096.0]):
        with pytest.raises(ValueError, match="length"):
            Au.melspectrogram(w, lengths=bad)
        with pytest.raises(ValueError, match="length"):
            Au.melspectrogram(w, lengths=torch.tensor(bad))
    with pytest.raises(_lib.NsgError, match="GPU tensor"):                            # everything valid but the device: no CPU fallback
        Au.melspectrogram(w, lengths=[4096, 513, 600])


def test_band_table_of_the_filterbank():
    """Each Slaney triangle is one contiguous run of bins and no row is empty, for every supported size; 22050 / 1024 / 80 has
    680 non-zeros of 41 040 in runs of 3 to 24 bins."""
    for n_fft in (512, 1024, 2048):
        for n_mels in (40, 80):
            basis, bands = Au.mel_basis(22050, n_fft, n_mels), Au._mel_bands(22050, n_fft, n_mels)
            assert bands.dtype == np.int32 and bands.shape == (n_mels, 2)
            for i, (f0, f1) in enumerate(bands):
                assert 0 <= f0 <= f1 <= n_fft // 2 and (basis[i, f0:f1 + 1] > 0).all()
                assert not basis[i, :f0].any() and not basis[i, f1 + 1:].any()
    bands = Au._mel_bands(22050, 1024, 80)
    runs = bands[:, 1] - bands[:, 0] + 1
    assert runs.sum() == 680 and runs.min() == 3 and runs.max() == 24


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """nsg_audio_melspectrogram / nsg_audio_preemphasis with pointers that are never dereferenced (the band table is host
    memory and real)."""
    lib = _lib.load()
    ok, null = 0x10000, 0
    bands = np.ascontiguousarray(Au._mel_bands(22050, 1024, 80))
    good = dict(wav=ok, lengths=0, basis=ok, bands=bands.ctypes.data, out=ok, B=2, L=4096, n_fft=1024, hop=256, n_mels=80, k=0.97,
                min_db=-100.0, ref_db=20.0, max_abs=1.0, frame_major=0)

    def mel(**change):
        a = dict(good, **change)
        p = [ctypes.c_void_p(a[k]) for k in ("wav", "lengths", "basis", "bands", "out")]
        return lib.nsg_audio_melspectrogram(*p, a["B"], a["L"], a["n_fft"], a["hop"], a["n_mels"], a["k"], a["min_db"], a["ref_db"], a["max_abs"],
                                            a["frame_major"], None)

    outside = bands.copy()
    outside[7, 1] = 513
    negative = bands.copy()
    negative[0, 0] = -1
    invalid = [dict(wav=null), dict(basis=null), dict(bands=null), dict(out=null), dict(B=0), dict(L=0), dict(L=-5), dict(hop=0), dict(n_mels=0),
               dict(max_abs=0.0), dict(min_db=0.0), dict(frame_major=2), dict(bands=outside.ctypes.data), dict(bands=negative.ctypes.data)]
    for change in invalid:
        assert mel(**change) == -1, change
        assert b"nsg_audio_melspectrogram" in lib.nsg_last_error_string()
    unsupported = [dict(n_fft=1000), dict(n_fft=256), dict(n_fft=4096), dict(L=512), dict(n_mels=129), dict(B=1 << 20, L=1 << 20, hop=1)]
    for change in unsupported:
        assert mel(**change) == -2, change
        assert b"nsg_audio_melspectrogram" in lib.nsg_last_error_string()
    p = ctypes.c_void_p
    for args in ((p(null), p(ok + 64), 1, 8), (p(ok), p(null), 1, 8), (p(ok), p(ok), 1, 8), (p(ok), p(ok + 64), 0, 8), (p(ok), p(ok + 64), 1, 0)):
        assert lib.nsg_audio_preemphasis(*args, 0.97, None) == -1, args
        assert b"nsg_audio_preemphasis" in lib.nsg_last_error_string()


def test_process_utterances_refuses_unusable_clips(tmp_path):
    from scipy.io import wavfile
    wavfile.write(str(tmp_path / "silent.wav"), 22050, np.zeros(4000, dtype=np.int16))
    wavfile.write(str(tmp_path / "short.wav"), 22050, np.ones(512, dtype=np.int16))
    for name in ("silent", "short"):
        with pytest.raises(ValueError, match=name):
            P.process_utterances([str(tmp_path / (name + ".wav"))], ["t"], str(tmp_path / "out"))
    with pytest.raises(ValueError):
        P.process_utterances([np.ones(4000, dtype=np.float32)], ["a", "b"], str(tmp_path / "out"))


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _ljspeech_tree(root, n=12, seed=0):
    """A synthetic LJSpeech tree: n int16 wavs of 0.3 - 1.2 s (tones under an envelope plus noise), metadata.csv."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "wavs"))
    lines, wavs = [], {}
    for i in range(n):
        L = int(rs.uniform(0.3, 1.2) * 22050)
        t = np.arange(L) / 22050
        y = sum(rs.rand() * np.sin(2 * np.pi * rs.uniform(100, 4000) * t + rs.rand() * 6.28) for _ in range(5))
        y = y * (0.5 + 0.5 * np.sin(2 * np.pi * rs.uniform(1, 5) * t)) + 0.05 * rs.randn(L)
        pcm = (y / np.abs(y).max() * rs.uniform(0.2, 0.9) * 32767).astype(np.int16)
        uid = "LJ001-%04d" % (i + 1)
        wavfile.write(os.path.join(root, "wavs", uid + ".wav"), 22050, pcm)
        wavs[i + 1] = pcm.astype(np.float32) / 32768.0
        lines.append("%s|Raw text %d|normalised text %d" % (uid, i, i))
    with open(os.path.join(root, "metadata.csv"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return wavs


@gpu
def test_build_from_path_writes_the_training_format(tmp_path):
    from neural_sound_generation_amd import models as M
    from neural_sound_generation_amd.optim import FlatAdam
    from neural_sound_generation_amd.train import FusedTrainStep, train_vqvae
    src = str(tmp_path / "LJSpeech-1.1")
    wavs = _ljspeech_tree(src)
    outs = {}
    for bc in (1, 5, 64):
        outs[bc] = str(tmp_path / ("out%d" % bc))
        meta = P.build_from_path(src, outs[bc], batch_clips=bc)
        assert len(meta) == 12
    root = outs[64]
    names = sorted(os.listdir(root))
    assert len(names) == 25 and "train.txt" in names
    for bc in (1, 5):
        assert sorted(os.listdir(outs[bc])) == names
        for nm in names:
            assert open(os.path.join(outs[bc], nm), "rb").read() == open(os.path.join(root, nm), "rb").read(), (bc, nm)
    rows = [ln.split("|") for ln in open(os.path.join(root, "train.txt"), encoding="utf-8").read().splitlines()]
    assert [tuple(r[:2]) + (int(r[2]), r[3]) for r in rows] == [tuple(m) for m in meta]
    for i, r in enumerate(rows, start=1):
        assert r[0] == "ljspeech-audio-%05d.npy" % i and r[1] == "ljspeech-mel-%05d.npy" % i and r[3] == "normalised text %d" % (i - 1)
        wav = wavs[i]
        wav = (wav / np.abs(wav).max() * 0.999).astype(np.float32)
        N = 1 + len(wav) // 256
        mel = np.load(os.path.join(root, r[1]), allow_pickle=False)
        assert mel.shape == (N, 80) and mel.dtype == np.float32 and mel.min() >= 0 and mel.max() <= 1
        H.check_amplitude(mel.T, wav, tag=r[1])
        audio = np.load(os.path.join(root, r[0]), allow_pickle=False)
        assert audio.dtype == np.float32 and audio.shape == (N * 256,) and int(r[2]) == N * 256
        assert (audio[:768] == 0).all() and np.array_equal(audio[768:], wav[:N * 256 - 768])
    # the loaders, and two steps each of both training paths
    loaders = Dm.get_data_loaders(root, batch_size=4, max_time_steps=64 * Dm.HOP_SIZE, num_workers=0, frame_multiple=4, with_audio=True)
    torch.manual_seed(1)
    model = M.VQVAE(1, 16, 32).to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3)

    class A:
        beta, log_interval, dataset = 1.0, 1000, "ljspeech"
    for epoch in range(2):
        assert np.isfinite(train_vqvae(A(), model, opt, Dm.DevicePrefetcher(loaders["train"], DEV), DEV, epoch))
    step = FusedTrainStep(model, optimizer=opt)
    n = 0
    for x, y, c, g_, lens in list(Dm.DevicePrefetcher(loaders["train"], DEV))[:2]:
        assert c.is_cuda and c.shape[1] == 80 and c.shape[2] % 4 == 0 and x.shape[2] == c.shape[2] * 256
        assert all(torch.isfinite(l).all() for l in step.step(c.unsqueeze(1)))
        n += 1
    assert n == 2


@gpu
def test_continue_audio():
    from neural_sound_generation_amd import models as M
    from neural_sound_generation_amd.evaluate import continue_audio
    from neural_sound_generation_amd.prior import GatedPixelCNN
    torch.manual_seed(2)
    vqvae = M.VQVAE(1, 32, 64).to(DEV).eval()
    prior = GatedPixelCNN(64, 16, 2, 4).to(DEV)
    B, keep, frames = 3, 18, 48
    label = torch.tensor([0, 2, 3], device=DEV)
    rs = np.random.RandomState(8)
    wav = torch.from_numpy(np.stack([H.rescale(rs.randn(256 * 31)) for _ in range(B)])).to(DEV)      # 32 frames
    u = torch.rand(B, frames, 513, generator=torch.Generator().manual_seed(5)).to(DEV)

    def run():
        return continue_audio(vqvae, prior, wav, label, keep, frames, generator=torch.Generator(device=DEV).manual_seed(7), angles0=u,
                              temperature=0.9, top_p=0.9)
    codes, mel, y = run()
    assert tuple(codes.shape) == (B, 20, frames // 4) and tuple(mel.shape) == (B, 1, 80, frames) and tuple(y.shape) == (B, 256 * (frames - 1))
    assert torch.isfinite(y).all()
    with torch.no_grad():
        known = vqvae.encode(Au.melspectrogram(wav).unsqueeze(1))
    assert torch.equal(codes[:, :, :keep // 4], known[:, :, :keep // 4])
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((codes, mel, y), again)), "deterministic under a fixed generator and angles0"
