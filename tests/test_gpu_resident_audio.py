"""GPU: the resident audio corpus -- nsg_collate_audio against its numpy restatement (tests/helpers/resident_audio_ref.py), by bits,
over every hop / T / B / alignment at which it takes another path, with NaN guards around `out`; offsets past 2^31 on both sides;
every refusal of its contract; data.ResidentMelCorpus.keep_audio and track_f0() from the resident samples against the tracks of
the files; the loaders with audio=True against data.get_data_loaders(with_audio=True) and against themselves without it; and
pitch-perturbed training (train.train_conditioned, epoch.run_conditioned_epoch) fed from the device against the host path."""
import functools
import os
import random
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, data as D, epoch as Ep, models as M, ops  # noqa: E402
from neural_sound_generation_amd import train as T_  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep  # noqa: E402
from tests.helpers import resident_audio_ref as R  # noqa: E402

DEV = "cuda:0"
NB, FMIN, FMAX = 8, 65.0, 500.0
F0 = {"n_bins": NB, "fmin": FMIN, "fmax": FMAX}
SPLIT = dict(test_size=0.25)                     # 8 clips: 6 train, 2 test
FRAMES = 997
NAN_BITS = 0x7FC0BEEF
GUARD = 16                                       # floats on either side of `out`


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def corpus_samples(hop):
    """997 frames x hop samples, finite random fp32 of both signs (no NaN: one found in `out` is a guard value that leaked)."""
    return np.random.RandomState(hop).uniform(-1, 1, FRAMES * hop).astype(np.float32)


def plan_for(B, T):
    """tests/test_gpu_resident_f0.py's: counts 0, 1, 3, 4, 13 and T (cut to T); starts of every residue mod 4; the last row ends on
    the corpus' last frame."""
    counts = [T, 0, 1, 3, 4, 13]
    plan = np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        plan[b] = (b, 20 * b + b % 4, min(counts[b % 6], T))
    plan[B - 1, 1] = FRAMES - plan[B - 1, 2]
    if B >= 7:
        assert sorted(set((plan[:, 1] % 4).tolist())) == [0, 1, 2, 3]
    return plan


def placed(values, shift):
    """`values` on the device as a slice of a larger tensor that starts `shift` floats past a 16-byte boundary."""
    big = torch.empty(len(values) + 8, dtype=torch.float32, device=DEV)
    t = big[4 + shift:4 + shift + len(values)]
    t.copy_(torch.from_numpy(values))
    assert t.data_ptr() % 16 == 4 * shift and t.is_contiguous()
    return t


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("T", [1, 5, 33])
@pytest.mark.parametrize("hop", [1, 3, 4, 256])
def test_kernel_is_the_restatement_at_every_alignment(hop, T, B):
    """hop 256, T 33 is 8 448 floats a row: two whole chunks of 4 096 (straight-line copies, or zeros behind a short row) and a cut
    one; with neither side on 16 bytes a chunk is 1 024 floats.  Every other case is the predicated path alone."""
    samples, plan = corpus_samples(hop), plan_for(B, T)
    want = torch.from_numpy(R.collate_audio(samples, plan, T, hop))
    assert plan[-1, 1] * hop + plan[-1, 2] * hop == len(samples)            # the last row ends on the corpus' last sample
    plan_dev, n = torch.from_numpy(plan).to(DEV), B * T * hop
    for corpus_shift in (0, 1):
        corpus = placed(samples, corpus_shift)
        for out_shift in (0, 1):
            buf = torch.empty(n + 2 * GUARD + 4, dtype=torch.int32, device=DEV).fill_(NAN_BITS).view(torch.float32)
            out = buf[GUARD + out_shift:GUARD + out_shift + n].view(B, T * hop)
            assert out.data_ptr() % 16 == 4 * out_shift
            got = ops.collate_audio(corpus, plan_dev, T, hop, out=out)
            assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (B, T * hop)
            assert torch.equal(bits(got).cpu(), bits(want)), (corpus_shift, out_shift)
            assert not bool(torch.isnan(got).any())
            guards = torch.cat((buf[:GUARD + out_shift], buf[GUARD + out_shift + n:])).view(torch.int32)
            assert bool((guards == NAN_BITS).all()), (corpus_shift, out_shift)
    # a plan on the host is checked, uploaded and gives the same
    assert torch.equal(bits(ops.collate_audio(corpus, torch.from_numpy(plan), T, hop)).cpu(), bits(want))


def test_what_the_loader_launches():
    """A small batch at hop 256 into a fresh tensor: both sides on 16 bytes, rows shorter and longer than a chunk's 4 096 floats."""
    hop, T = 256, 20
    samples = corpus_samples(hop)
    plan = np.array([[0, 3, 20], [1, 100, 16], [2, FRAMES - 12, 12]], dtype=np.int64)
    corpus = torch.from_numpy(samples).to(DEV)
    got = ops.collate_audio(corpus, torch.from_numpy(plan).to(DEV), T)
    assert corpus.data_ptr() % 16 == 0 and got.data_ptr() % 16 == 0 and got.dtype == torch.float32 and tuple(got.shape) == (3, T * hop)
    assert torch.equal(bits(got).cpu(), bits(torch.from_numpy(R.collate_audio(samples, plan, T, hop))))


def test_offsets_past_2_to_the_31_on_both_sides():
    """A corpus and an `out` of 2^31 + 2^20 floats each (8.6 GB): the last row copies the corpus' last 4 096 frames into the last
    2^20 elements of out; every other row has count 0 and is zeros.  Only what is compared is initialised or read back."""
    hop, T, B = 256, 4096, 2049
    L = T * hop
    n = (1 << 31) + L
    corpus = torch.empty(n, dtype=torch.float32, device=DEV)
    tail = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, L).astype(np.float32))
    corpus[-L:] = tail.to(DEV)
    corpus[-L - 1024:-L] = 7.0                                                 # (what a 32-bit offset, or one frame too few, would show)
    plan = np.zeros((B, 3), dtype=np.int64)
    plan[:, 0], plan[:, 1] = np.arange(B), np.arange(B) * T
    plan[-1] = (B - 1, n // hop - T, T)
    out = torch.empty(B, L, dtype=torch.float32, device=DEV)
    probe = [0, 1, B - 3, B - 2]
    out[probe] = float("nan")
    got = ops.collate_audio(corpus, torch.from_numpy(plan), T, hop, out=out)
    assert torch.equal(bits(got[-1]).cpu(), bits(tail))
    assert bool((bits(got[probe]) == 0).all())                                # +0.0, bit for bit
    del corpus, out, got
    torch.cuda.empty_cache()


def test_every_refusal_leaves_out_untouched():
    hop, B, T = 256, 4, 26
    corpus = torch.from_numpy(corpus_samples(hop)).to(DEV)
    plan = torch.from_numpy(plan_for(B, T)).to(DEV)
    out = torch.full((B, T * hop), -7.0, device=DEV)
    p = lambda t, off=0: c_void_p(t.data_ptr() + off)                           # noqa: E731
    null = c_void_p(0)
    base = dict(corpus=p(corpus), samples=FRAMES * hop, hop=hop, plan=p(plan), B=B, T=T, out=p(out))

    def call(**kw):
        a = dict(base, **kw)
        _lib.call("nsg_collate_audio", a["corpus"], a["samples"], a["hop"], a["plan"], a["B"], a["T"], a["out"], ops._stream())
    bad = [dict(corpus=null), dict(plan=null), dict(out=null),
           dict(B=0), dict(B=-1), dict(T=0), dict(T=-26), dict(hop=0), dict(hop=-256),
           dict(samples=-1),
           dict(T=1 << 23), dict(T=2, hop=1 << 30), dict(T=(1 << 31) - 1, hop=(1 << 31) - 1),
           dict(corpus=p(corpus, 2)), dict(out=p(out, 1)), dict(out=p(out, 2)), dict(plan=p(plan, 4))]
    for kw in bad:
        with pytest.raises(_lib.NsgError, match="nsg_collate_audio"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    call()                                                                      # (the unchanged arguments are served)
    assert not bool((out == -7.0).any())
    # the wrapper's own
    with pytest.raises(_lib.NsgError, match="does not hold"):
        ops.collate_audio(corpus, plan, T, hop, out=out[:, 1:].contiguous())
    with pytest.raises(_lib.NsgError, match="collate plan"):
        ops.collate_audio(corpus, torch.tensor([[0, FRAMES - 3, 4]]), T, hop)


# ---- the corpus -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    """8 voiced clips of 40 .. 90 frames, two speakers; the train split holds 6 of them, two longer than 64 frames."""
    path = str(tmp_path_factory.mktemp("resident_audio") / "root")
    D.write_synthetic_data_root(path, n_utts=8, min_frames=40, max_frames=90, n_speakers=2, seed=11, voiced=True)
    return path


def sources(root, train=True):
    kw = dict(train=train, **SPLIT)
    return D.MelSpecDataSource(root, **kw), D.RawAudioDataSource(root, **kw)


def test_keep_audio_on_the_device_is_the_files(root):
    mel, wav = sources(root)
    c = D.ResidentMelCorpus(mel, DEV).keep_audio(wav)
    assert c.audio.device == c.frames.device and c.audio.dtype == torch.float32 and c.audio_hop == 256
    want = np.concatenate([np.load(p) for p in wav.paths])
    assert torch.equal(bits(c.audio).cpu(), bits(torch.from_numpy(want)))


@pytest.mark.parametrize("group_clips", [1, 3, 64])
@pytest.mark.parametrize("tracker", ["yin", "viterbi"])
def test_track_from_the_resident_audio_is_the_track_from_the_files(root, tracker, group_clips):
    mel, wav = sources(root)
    files = D.ResidentMelCorpus(mel, DEV).track_f0(wav, tracker=tracker, group_clips=group_clips)
    res = D.ResidentMelCorpus(mel, DEV).keep_audio(wav)
    assert res.track_f0(tracker=tracker, group_clips=group_clips) is res
    assert torch.equal(bits(res.f0), bits(files.f0)) and np.array_equal(res.f0_sums, files.f0_sums) and res.f0_settings == files.f0_settings
    assert 2 * int((res.f0 > 0).sum()) >= res.f0.numel()                       # a voiced root: the equality is not one of zeros
    if group_clips == 3:                                                        # the sample bound cuts the groups as well
        again = D.ResidentMelCorpus(mel, DEV).keep_audio(wav).track_f0(tracker=tracker, group_samples=40000)
        assert torch.equal(bits(again.f0), bits(files.f0)) and np.array_equal(again.f0_sums, files.f0_sums)


# ---- the loaders ------------------------------------------------------------------------------------------------------------
MAX_STEPS = 64 * 256


def seeded(seed):
    random.seed(seed)
    np.random.seed(seed)


def resident(root, f0=None, audio=True):
    return D.get_resident_loaders(root, 3, max_time_steps=MAX_STEPS, frame_multiple=4, device=DEV, f0=f0, audio=audio, **SPLIT)


def host(root):
    return D.get_data_loaders(root, 3, max_time_steps=MAX_STEPS, num_workers=0, with_audio=True, frame_multiple=4, pin_memory=False, **SPLIT)


@pytest.fixture(scope="module")
def loaders(root):
    return {"audio": resident(root), "plain": resident(root, audio=False), "audio_f0": resident(root, f0=F0), "f0": resident(root, f0=F0, audio=False)}


@pytest.mark.parametrize("phase", ["train", "test"])
def test_batches_are_the_host_loader_s(root, loaders, phase):
    ld = loaders["audio"][phase]
    assert ld.audio and ld.dataset.audio is not None and ld.dataset.f0 is None and not loaders["plain"][phase].audio
    assert loaders["plain"][phase].dataset.audio is None
    seeded(5)
    want = list(host(root)[phase])
    after = (random.random(), np.random.rand())
    seeded(5)
    got = list(ld)
    assert (random.random(), np.random.rand()) == after                        # the same draws
    seeded(5)
    plain = list(loaders["plain"][phase])
    assert (random.random(), np.random.rand()) == after
    assert len(got) == len(want) == len(plain) == (2 if phase == "train" else 1)
    if phase == "test":
        assert len(got[-1][2]) == 2                                             # a short last batch
    cropped = whole = 0
    for h, r, p in zip(want, got, plain):
        assert len(r) == 5 and len(p) == 5
        x, y, c, g, lengths = r
        T = c.shape[2]
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (len(c), 1, T * 256) and tuple(y.shape) == (len(c), T * 256, 1)
        assert x.is_contiguous() and y.is_contiguous() and x.data_ptr() == y.data_ptr()
        assert x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr()
        assert torch.equal(bits(x).cpu(), bits(h[0])) and torch.equal(bits(y).cpu(), bits(h[1]))
        assert torch.equal(bits(c).cpu(), bits(h[2])) and torch.equal(g.cpu(), h[3]) and torch.equal(lengths, h[4])
        # without audio: today's batches
        assert p[0] is None and p[1] is None
        assert torch.equal(bits(p[2]), bits(c)) and torch.equal(p[3], g) and torch.equal(p[4], lengths)
        cropped += int((lengths == MAX_STEPS).sum())
        whole += int((lengths < MAX_STEPS).sum())
        assert T % 4 == 0 and bool((lengths % (4 * 256) == 0).all())
    if phase == "train":
        assert cropped >= 1 and whole >= 1                                      # some clips are cropped and some are not


@pytest.mark.parametrize("phase", ["train", "test"])
def test_bins_beside_the_audio_are_the_bins_without_it(loaders, phase):
    both, only = loaders["audio_f0"][phase], loaders["f0"][phase]
    assert both.dataset.audio is not None and only.dataset.audio is None
    assert torch.equal(bits(both.dataset.f0), bits(only.dataset.f0))           # tracked from the resident samples / from the files
    seeded(7)
    six = list(both)
    seeded(7)
    ref = list(only)
    seeded(7)
    five = list(loaders["audio"][phase])
    assert len(six) == len(ref) == len(five) > 0
    for a, b, c in zip(six, ref, five):
        assert len(a) == 6 and len(b) == 6 and b[0] is None and a[0] is not None
        assert a[5].dtype == torch.int64 and torch.equal(a[5], b[5]) and torch.equal(bits(a[2]), bits(b[2])) and torch.equal(a[4], b[4])
        assert torch.equal(bits(a[0]), bits(c[0])) and torch.equal(a[3], b[3])
    assert any(int(a[5].max()) > 0 for a in six)


# ---- the consumers ----------------------------------------------------------------------------------------------------------
class Args:
    log_interval, model, dataset, dim, z_dim = 1, "vqvae", "synth", 16, 32


class Fixed(list):
    """An epoch's batches, kept so that they can be fed twice."""
    dataset = range(6)


def fresh(seed=1):
    torch.manual_seed(seed)
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=NB).to(DEV).train()
    return model, FusedTrainStep(model, lr=1e-3)


def gen(seed=3):
    return torch.Generator().manual_seed(seed)


def same_model(a, b):
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k


def test_perturbed_epoch_from_the_device_is_the_host_path_s(root, loaders):
    """No f0=: the bins are tracked from x on both sides, so everything the step sees is equal, and (the step is
    reproducible) so are the loss and every parameter after the epoch."""
    seeded(3)
    from_device = Fixed(loaders["audio"]["train"])
    seeded(3)
    from_host = Fixed(host(root)["train"])
    assert len(from_device) == len(from_host) == 2
    model_d, step_d = fresh()
    model_h, step_h = fresh()
    same_model(model_d, model_h)
    before = {k: v.clone() for k, v in model_d.state_dict().items()}
    loss_d = T_.train_conditioned(Args(), model_d, step_d, from_device, DEV, 0, pitch_perturb=(-4, 4), generator=gen())
    loss_h = T_.train_conditioned(Args(), model_h, step_h, from_host, DEV, 0, pitch_perturb=(-4, 4), generator=gen())
    assert np.isfinite(loss_d) and np.float64(loss_d).tobytes() == np.float64(loss_h).tobytes()
    same_model(model_d, model_h)
    assert any(not torch.equal(v, before[k]) for k, v in model_d.state_dict().items()) and step_d.opt.step_count == 2


def test_perturbed_epoch_with_the_resident_track(loaders):
    seeded(3)
    batches = Fixed(loaders["audio_f0"]["train"])
    assert all(len(b) == 6 and b[0] is not None for b in batches)
    model_p, step_p = fresh()
    model_u, step_u = fresh()
    moved = T_.train_conditioned(Args(), model_p, step_p, batches, DEV, 0, pitch_perturb=(-4, 4), generator=gen())
    plain = T_.train_conditioned(Args(), model_u, step_u, batches, DEV, 0)
    assert np.isfinite(moved) and np.isfinite(plain) and moved != plain
    # without audio=True the loop still says what it lacks
    seeded(3)
    with pytest.raises(ValueError, match="without audio=True keeps no audio"):
        T_.train_conditioned(Args(), model_u, step_u, Fixed(loaders["f0"]["train"]), DEV, 0, pitch_perturb=(-4, 4))


def test_run_conditioned_epoch_with_the_perturbation(loaders, tmp_path):
    args = Args()
    args.sampledir = str(tmp_path / "samples")
    seeded(4)
    ld = loaders["audio_f0"]
    model, step = fresh(5)
    ckpt = str(tmp_path / "models" / "ckpt.pth.tar")
    out = Ep.run_conditioned_epoch(args, model, step, ld["train"], ld["test"], DEV, 1, checkpoint_path=ckpt, pitch_perturb=(-4, 4), generator=gen())
    assert set(out) == {"train_loss", "test_loss_recons", "test_loss_vq", "reconstruction", "wav", "checkpoint"}
    assert all(os.path.exists(out[k]) for k in ("reconstruction", "wav", "checkpoint")) and out["checkpoint"] == ckpt
    assert np.isfinite([out["train_loss"], out["test_loss_recons"], out["test_loss_vq"]]).all() and step.opt.step_count == 2
    # the training half is train_conditioned's under the same arguments
    seeded(4)
    model2, step2 = fresh(5)
    assert T_.train_conditioned(args, model2, step2, ld["train"], DEV, 1, pitch_perturb=(-4, 4), generator=gen()) == out["train_loss"]
    same_model(model, model2)
