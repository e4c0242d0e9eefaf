"""CPU: the resident F0 corpus' host side -- nsg_collate_f0_bins' ABI and refusals (fake pointers, nothing launched), its numpy
restatement (tests/helpers/resident_f0_ref.py) against hand-made plans, the voiced synthetic data root (today's bytes without
it; the mels untouched with it; enough voiced columns and distinct bins, by the YIN restatement, for the GPU tests not to be
vacuous), and the ValueErrors and the six-tuple feed of the Python layers before a device is touched."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, data as D, epoch, evaluate, models, ops, train
from tests.helpers import f0_cond_ref, f0_ref, resident_f0_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004), ctypes.c_void_p(0)
NAME = "nsg_collate_f0_bins"


def test_symbol_is_declared_exported_and_takes_no_workspace():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    assert re.search(r"NSG_API\s+int\s+%s\s*\(" % NAME, text)
    assert NAME in _lib.HEADER_SYMBOLS and hasattr(_lib.load(), NAME)
    sigs, _, _ = _lib.parse_header(text)
    V, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert sigs[NAME] == (I32, [V, I64, V, V, V, V, V] + [I32] * 4 + [F32] * 2 + [V])
    assert ctypes.c_size_t not in sigs[NAME][1]


def test_launcher_refuses_before_any_launch():
    lib = _lib.load()

    def call(corpus=P, frames=997, plan=P, affine=NULL, bins=P, logf=NULL, f0_out=NULL, B=4, T=26, W=6, n_bins=8, fmin=65.0, fmax=500.0):
        return lib.nsg_collate_f0_bins(corpus, frames, plan, affine, bins, logf, f0_out, B, T, W, n_bins, fmin, fmax, None)

    odd2 = ctypes.c_void_p(0x10002)
    nan, inf = float("nan"), float("inf")
    # two neighbouring fp32 frequencies whose log2 rounds to one fp32 value (an ulp of f near 100 moves log2 f by a quarter ulp)
    same = [(float(f), float(np.nextafter(f, np.float32(1e3)))) for f in np.arange(100, 120, dtype=np.float32)]
    below, above = next((f, g) for f, g in same if np.float32(np.log2(f)) == np.float32(np.log2(g)))
    assert above > below
    bad = [dict(corpus=NULL), dict(plan=NULL), dict(bins=NULL),                                        # null pointers
           dict(B=0), dict(T=0), dict(W=0), dict(B=-1), dict(T=-4), dict(W=-1),                         # non-positive sizes
           dict(W=7), dict(T=23),                                                                      # T < 4 W
           dict(n_bins=0), dict(n_bins=-1),
           dict(fmin=0.0), dict(fmin=-65.0), dict(fmin=500.0), dict(fmin=600.0), dict(fmin=nan), dict(fmax=nan), dict(fmax=inf),
           dict(fmin=below, fmax=above),                                                                # one value in fp32 log2
           dict(frames=-1),
           dict(corpus=odd2), dict(affine=odd2), dict(logf=odd2), dict(f0_out=odd2), dict(plan=ODD), dict(bins=ODD),     # misaligned
           dict(B=1 << 16, T=1 << 15, W=8)]                                                            # B T >= 2^31
    for kw in bad:
        assert call(**kw) == -1 and NAME.encode() in lib.nsg_last_error_string(), kw


def test_restatement_on_hand_made_plans():
    # 12 corpus frames: an unvoiced frame, in-range values, one below fmin and one above fmax
    corpus = np.array([0, 100, 100, 200, 200, 0, 0, 400, 30, 30, 1000, 1000], dtype=np.float32)
    plan = np.array([[0, 0, 8], [1, 1, 4], [2, 8, 4], [3, 10, 8], [4, 4, 3], [5, -2, 6], [6, 0, 99], [7, 3, 0]], dtype=np.int64)
    rows, count = R.gather(corpus, plan, 8)
    assert count.tolist() == [8, 4, 4, 8, 3, 6, 8, 0]
    assert rows[0].tolist() == corpus[:8].tolist()
    assert rows[1].tolist() == [100, 100, 200, 200, 0, 0, 0, 0]
    assert rows[3].tolist() == [1000, 1000, 0, 0, 0, 0, 0, 0]                      # past the corpus' end: zeros
    assert rows[5].tolist() == [0, 0, 0, 100, 100, 200, 0, 0]                      # before its start: zeros
    assert rows[6].tolist() == corpus[:8].tolist() and not rows[7].any()           # count clamped to T; an empty item
    bins, logf, rows2 = R.collate_bins_f32(corpus, plan, 8, 4, 65.0, 500.0)
    assert np.array_equal(rows, rows2) and bins.shape == (8, 2) and logf.dtype == np.float32
    # item 0: {100, 100, 200} -> mean log2 = (2 log2 100 + log2 200) / 3, bin 1 + floor(4 (l - log2 65) / log2 (500 / 65));
    # then {200, 400}: 3 voiced of 4 and 2 of 4
    for w, vals in ((0, [100, 100, 200]), (1, [200, 400])):
        l = np.mean(np.log2(vals))
        assert bins[0, w] == 1 + int(np.floor(4 * (l - np.log2(65.0)) / np.log2(500.0 / 65.0))) and abs(logf[0, w] - l) < 1e-6
    assert bins[1].tolist() == [bins[1, 0], 0] and bins[1, 0] >= 1                 # the second column lies past count
    assert bins[2].tolist() == [2, 0]                                              # {30, 30, 1000, 1000}: mean log2 = 7.44, the second step
    assert bins[3].tolist() == [4, 0] and bins[7].tolist() == [0, 0]               # above fmax: clamped to the top bin
    assert bins[4, 0] == 0                                                         # {200, 0, 0}: one voiced frame is no column
    # the rule itself is nsg_f0_bins' restatement on the gathered rows
    want, want_l = f0_cond_ref.bins_f32(rows, 2, 4, 65.0, 500.0, frames=count)
    assert np.array_equal(bins, want) and np.array_equal(logf, want_l)
    one = R.collate_bins_f32(corpus, plan, 8, 4, 65.0, 500.0, W=1)[0]              # W < T // 4: the leading columns
    assert np.array_equal(one, bins[:, :1])
    assert R.interior(32).nonzero()[0].tolist() == list(range(2, 29))              # frames 2 .. count - 4 at the defaults
    assert not R.interior(5).any()


def _todays_root(root, n_utts, min_frames, max_frames, n_speakers, seed):
    """write_synthetic_data_root's draws as they were before `voiced` existed, restated inline -> {file name: bytes}."""
    import io
    rs = np.random.RandomState(seed)
    files, lines = {}, []

    def dump(a):
        b = io.BytesIO()
        np.save(b, a, allow_pickle=False)
        return b.getvalue()
    for i in range(n_utts):
        frames = int(rs.randint(min_frames, max_frames + 1))
        files["synth-mel-%05d.npy" % i] = dump(rs.rand(frames, 80).astype(np.float32))
        files["synth-audio-%05d.npy" % i] = dump(rs.uniform(-1, 1, frames * 256).astype(np.float32))
        lines.append("|".join(["synth-audio-%05d.npy" % i, "synth-mel-%05d.npy" % i, str(frames * 256), "utterance %d" % i,
                               str(int(rs.randint(0, n_speakers)))]))
    files["train.txt"] = ("\n".join(lines) + "\n").encode("utf-8")
    return files


def _read(root):
    return {f: open(os.path.join(root, f), "rb").read() for f in sorted(os.listdir(root))}


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("roots")
    plain, voiced = str(base / "plain"), str(base / "voiced")
    D.write_synthetic_data_root(plain, n_utts=3, min_frames=40, max_frames=60, n_speakers=2, seed=5)
    D.write_synthetic_data_root(voiced, n_utts=3, min_frames=40, max_frames=60, n_speakers=2, seed=5, voiced=True)
    return plain, voiced


def test_unvoiced_root_is_todays_bytes(roots, tmp_path):
    want = _todays_root(None, 3, 40, 60, 2, 5)
    assert _read(roots[0]) == want
    explicit = str(tmp_path / "explicit")
    D.write_synthetic_data_root(explicit, n_utts=3, min_frames=40, max_frames=60, n_speakers=2, seed=5, voiced=False)
    assert _read(explicit) == want


def test_voiced_root_changes_the_audio_alone(roots):
    plain, voiced = _read(roots[0]), _read(roots[1])
    assert sorted(plain) == sorted(voiced)
    for name in plain:
        assert (plain[name] == voiced[name]) == ("audio" not in name), name
    for i in range(3):
        mel = np.load(os.path.join(roots[1], "synth-mel-%05d.npy" % i))
        wav = np.load(os.path.join(roots[1], "synth-audio-%05d.npy" % i))
        n = len(mel) * 256
        assert wav.dtype == np.float32 and wav.shape == (n,)
        # the recipe, restated: harmonics of a glide from f to 1.3 f, f = 110 (1 + 0.25 (i mod 4)); a quiet noise tail
        f = 110.0 * (1 + 0.25 * (i % 4)) * (1 + 0.3 * np.arange(n) / n)
        phase = np.cumsum(2 * np.pi * f / 22050.0)
        tone = 0.3 * sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7))
        assert np.array_equal(wav[:n - n // 5], tone[:n - n // 5].astype(np.float32))
        tail = wav[n - n // 5:]
        assert 0.004 < float(tail.std()) < 0.008 and float(np.abs(wav[:n - n // 5]).max()) > 0.2


def test_voiced_root_has_voiced_columns_and_distinct_bins(roots):
    """The condition the GPU tests rely on, by the YIN restatement: at least half of the latent columns of the 3-clip root are
    voiced and at least 3 distinct non-zero bins occur (8 bins over 65 .. 500 Hz)."""
    voiced = total = 0
    seen = set()
    for i in range(3):
        wav = np.load(os.path.join(roots[1], "synth-audio-%05d.npy" % i))
        frames = len(wav) // 256
        f0, _ = f0_ref.yin_f32(wav)
        assert len(f0) == frames + 1
        W = frames // 4
        bins, _ = f0_cond_ref.bins_f32(f0[None, :4 * W], W, 8, 65.0, 500.0)
        voiced, total = voiced + int((bins > 0).sum()), total + W
        seen |= set(bins[bins > 0].tolist())
    assert 2 * voiced >= total, (voiced, total)
    assert len(seen) >= 3, seen


def test_python_layers_raise_on_the_cpu_before_touching_a_device(roots):
    z = torch.zeros(12)
    plan = torch.tensor([[0, 0, 8]])
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.collate_f0_bins(z, plan, 8, 8, 65.0, 500.0)
    with pytest.raises(_lib.NsgError, match="past the corpus"):                    # a host plan is checked before anything else
        ops.collate_f0_bins(z, torch.tensor([[0, 8, 8]]), 8, 8, 65.0, 500.0)
    with pytest.raises(_lib.NsgError, match=r"not \(frames,\)"):
        ops.collate_f0_bins(torch.zeros(3, 4), plan, 8, 8, 65.0, 500.0)
    with pytest.raises(_lib.NsgError, match="plan: expected torch.int64"):
        ops.collate_f0_bins(z, plan.to(torch.int32), 8, 8, 65.0, 500.0)
    kw = dict(train=True, test_size=0.34)
    corpus = D.ResidentMelCorpus(D.MelSpecDataSource(roots[1], **kw), device="cpu")
    assert corpus.f0 is None and corpus.f0_sums is None and corpus.f0_settings is None
    with pytest.raises(ValueError, match="without an F0 track"):
        D.ResidentMelLoader(corpus, 2, f0=(8, 65.0, 500.0))
    for bad in ((8, 65.0), (0, 65.0, 500.0), (8.0, 65.0, 500.0), (8, 500.0, 65.0), (8, 0.0, 500.0)):
        with pytest.raises(ValueError, match="n_bins, fmin, fmax"):
            D.ResidentMelLoader(corpus, 2, f0=bad)
    with pytest.raises(ValueError, match="no F0 track"):
        corpus.speaker_f0_stats(2)
    audio_src = D.RawAudioDataSource(roots[1], **kw)
    with pytest.raises(ValueError, match="tracker must be"):
        corpus.track_f0(audio_src, tracker="pyin")
    with pytest.raises(ValueError, match="tracker_options"):
        corpus.track_f0(audio_src, tracker_options={"jump_cost": 0.2})
    with pytest.raises(ValueError, match="not the same split"):
        corpus.track_f0(D.RawAudioDataSource(roots[1], train=False, test_size=0.34))
    with pytest.raises(ValueError, match="n_bins, fmin, fmax"):
        D.get_resident_loaders(roots[1], 2, f0={"n_bins": 8})
    with pytest.raises(ValueError, match="n_bins, fmin, fmax"):
        D.get_resident_loaders(roots[1], 2, f0={"n_bins": 8, "fmin": 65.0, "fmax": 500.0, "threshold": 0.2})
    assert D.ResidentMelLoader(corpus, 2).f0 is None


class _Step:
    """A stand-in for FusedTrainStep on the CPU: records what train_conditioned feeds it."""

    def __init__(self):
        self.fed = []

    def step(self, c, g=None, f0_bins=None):
        self.fed.append((c, g, f0_bins))
        return torch.tensor(1.0), torch.tensor(0.5), torch.tensor(0.25)


def test_train_conditioned_feeds_a_sixth_element_as_it_comes():
    args = types.SimpleNamespace(log_interval=1)
    cpu = torch.device("cpu")
    with_f0 = models.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8)
    without = models.VQVAE(1, 16, 32, n_speakers=2)
    c, g, lens = torch.rand(2, 80, 32), torch.tensor([0, 1]), torch.tensor([8192, 8192])
    bins = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [8, 0, 0, 1, 1, 2, 2, 3]])

    class Loader(list):
        dataset = [0, 1]
    step = _Step()
    loss = train.train_conditioned(args, with_f0, step, Loader([(None, None, c, g, lens, bins)]), cpu, 0)
    assert loss == 1.5 and len(step.fed) == 1
    c_fed, g_fed, b_fed = step.fed[0]
    assert torch.equal(c_fed, c.unsqueeze(1)) and torch.equal(g_fed, g) and torch.equal(b_fed, bins)
    # a model without an F0 table is not given them; a five-tuple without audio still cannot feed one that has it
    step = _Step()
    train.train_conditioned(args, without, step, Loader([(None, None, c, g, lens, bins)]), cpu, 0)
    assert step.fed[0][2] is None and torch.equal(step.fed[0][1], g)
    for fn in (lambda b: train.train_conditioned(args, with_f0, _Step(), Loader([b]), cpu, 0),
               lambda b: evaluate.test_conditioned(args, with_f0, Loader([b]), cpu, 0),
               lambda b: epoch.run_conditioned_epoch(args, with_f0, types.SimpleNamespace(opt=None, step=None), Loader([b]), Loader([b]), cpu, 0)):
        with pytest.raises(ValueError, match=r"get_data_loaders\(with_audio=True\)"):
            fn((None, None, c, g, lens))
    with pytest.raises(ValueError, match="tracker must be"):
        evaluate.test_conditioned(args, with_f0, Loader([]), cpu, 0, tracker="pyin")
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.test_conditioned(args, with_f0, Loader([]), cpu, 0)
