"""The resident loader's host side (data.ResidentMelCorpus on the CPU, plan_batch, ResidentMelLoader.plan_epoch, ops.collate_mels'
refusals) without a GPU: an epoch's plan, applied with numpy indexing to the concatenated corpus, is the host loader's epoch
(DataLoader + MelDataset + Collate), bit for bit -- c, g and input_lengths, batch for batch -- when both draw from equal seeds."""
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from neural_sound_generation_amd import _lib, data as Dm, ops

HOP = Dm.HOP_SIZE
BS = 8


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("resident") / "arctic")
    # seed 27: clips of 2, 3, 4 and 5 frames are among the 37 (the default seed's shortest clip has 4)
    Dm.write_synthetic_data_root(r, n_utts=37, min_frames=2, max_frames=200, n_speakers=3, with_audio=False, seed=27)
    return r


def whole(root):
    """All 37 utterances as one source, for the train phase's sampler and the test phase's sequential order alike (the
    train / test split is get_resident_loaders' business: tests/test_gpu_resident_loader.py)."""
    class All(Dm.MelSpecDataSource):
        def interest_indices(self, n):
            return np.arange(n)
    return All(root)


def host_epoch(mel, train, max_time_steps, fm, seed):
    ds = Dm.MelDataset(mel)
    sampler = Dm.PartialyRandomizedSimilarTimeLengthSampler(ds.lengths, batch_size=BS) if train else None
    loader = DataLoader(ds, batch_size=BS, sampler=sampler, shuffle=False, num_workers=0,
                        collate_fn=Dm.Collate(max_time_steps, frame_multiple=fm, rng=np.random.RandomState(7)))
    random.seed(seed)
    return [(c.numpy(), None if g is None else g.numpy(), lens.numpy()) for _, _, c, g, lens in loader]


def apply_plan(corpus, ep, k):
    """Batch k of an epoch plan by numpy indexing: what nsg_collate_mels is specified to write."""
    frames = corpus.frames.numpy()
    B, T = int(ep.sizes[k]), int(ep.widths[k])
    c = np.zeros((B, Dm.NUM_MELS, T), dtype=np.float32)
    for b in range(B):
        _, start, count = ep.plan[k, b]
        c[b, :, :count] = frames[start:start + count].T
    g = corpus.speaker_ids.numpy()[ep.plan[k, :B, 0]] if corpus.speaker_ids is not None else None
    return c, g, ep.plan[k, :B, 2] * HOP


@pytest.fixture(scope="module")
def corpus(root):
    return Dm.ResidentMelCorpus(whole(root), "cpu")


def test_corpus_is_the_files_concatenated(root, corpus):
    mel = whole(root)
    assert len(corpus) == 37 and corpus.frames.dtype == torch.float32 and tuple(corpus.frames.shape) == (int(corpus.offsets[-1]), 80)
    assert corpus.lengths == mel.lengths and np.array_equal(corpus.n_frames * HOP, np.array(mel.lengths))
    assert corpus.n_frames.min() == 2                                     # the root does hold clips shorter than frame_multiple = 4
    for i, p in enumerate(mel.paths):
        assert np.array_equal(corpus.frames[corpus.offsets[i]:corpus.offsets[i + 1]].numpy(), np.load(p))
    assert corpus.speaker_ids.dtype == torch.int64 and corpus.speaker_ids.tolist() == mel.speaker_ids


def test_corpus_staging_in_chunks(root, corpus, monkeypatch):
    monkeypatch.setattr(Dm.ResidentMelCorpus, "CHUNK_FRAMES", 37)        # clips cross chunk edges; the last chunk is partial
    again = Dm.ResidentMelCorpus(whole(root), "cpu")
    assert torch.equal(again.frames, corpus.frames)


def test_corpus_refuses_a_wrong_shape(tmp_path):
    r = str(tmp_path / "bad")
    Dm.write_synthetic_data_root(r, n_utts=4, with_audio=False)
    np.save(r + "/synth-mel-00002.npy", np.zeros((10, 79), np.float32))
    with pytest.raises(ValueError, match="expected a .frames, 80. array"):
        Dm.ResidentMelCorpus(whole(r), "cpu")


@pytest.mark.parametrize("fm", [1, 4])
@pytest.mark.parametrize("max_time_steps", [None, 64 * 256, 100 * 256 + 17])
@pytest.mark.parametrize("train", [True, False])
def test_epoch_equals_the_host_loader(root, corpus, train, max_time_steps, fm):
    want = host_epoch(whole(root), train, max_time_steps, fm, seed=11)
    loader = Dm.ResidentMelLoader(corpus, BS, max_time_steps, fm, train=train, rng=np.random.RandomState(7))
    random.seed(11)
    ep = loader.plan_epoch()
    ops.check_collate_plan(ep.plan, ep.widths[:, None], len(corpus.frames))
    assert len(ep) == len(want) == len(loader) == 5 and ep.sizes.tolist() == [8, 8, 8, 8, 5]
    assert sorted(ep.plan[k, b, 0] for k in range(5) for b in range(ep.sizes[k])) == list(range(37))    # every utterance once
    cropped = 0
    for k, (c, g, lens) in enumerate(want):
        got_c, got_g, got_lens = apply_plan(corpus, ep, k)
        assert got_c.shape == c.shape and np.array_equal(got_c, c), k
        assert np.array_equal(got_g, g) and got_g.dtype == g.dtype == np.int64, k
        assert np.array_equal(got_lens, lens) and got_lens.dtype == lens.dtype == np.int64, k
        cropped += int((ep.plan[k, :, 1] != corpus.offsets[ep.plan[k, :, 0]]).sum())
    if max_time_steps is not None:
        assert cropped > 0                                                # random crops were drawn, and drawn alike
    if fm == 4:
        counts = np.concatenate([ep.plan[k, :ep.sizes[k], 2] for k in range(5)])
        assert (counts[counts >= 4] % 4 == 0).all() and (counts < 4).any()     # the "shorter than frame_multiple" rule ran


def test_a_second_epoch_is_another_order(corpus):
    loader = Dm.ResidentMelLoader(corpus, BS, 64 * 256, 4, rng=np.random.RandomState(7))
    random.seed(3)
    a, b = loader.plan_epoch(), loader.plan_epoch()
    assert not np.array_equal(a.plan, b.plan)
    for ep in (a, b):
        assert sorted(ep.plan[k, i, 0] for k in range(5) for i in range(ep.sizes[k])) == list(range(37))


def test_plan_batch_consumes_the_rng_as_collate_does():
    n_frames = [2, 300, 64, 65, 199, 3, 1000]
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    s, count = Dm.plan_batch(n_frames, 64 * 256 + 100, 256, 4, a)
    batch = [(None, np.arange(n, dtype=np.float32)[:, None].repeat(80, 1), None) for n in n_frames]
    _, _, c, _, lens = Dm.Collate(64 * 256 + 100, frame_multiple=4, rng=b)(batch)
    assert a.randint(1 << 30) == b.randint(1 << 30)                      # the same number of draws
    assert count.tolist() == [2, 64, 64, 64, 64, 3, 64] and np.array_equal(count * 256, lens.numpy())
    for i in range(len(n_frames)):
        assert np.array_equal(c[i, 0, :count[i]].numpy(), np.arange(s[i], s[i] + count[i], dtype=np.float32))


@pytest.mark.parametrize("world", [2, 3])
def test_shards(corpus, world):
    def epoch(shard):
        random.seed(21)
        return Dm.ResidentMelLoader(corpus, BS, 64 * 256, 4, rng=np.random.RandomState(7), shard=shard)

    full = epoch(None).plan_epoch()
    kept = 5 // world * world
    shards = []
    for rank in range(world):
        loader = epoch((rank, world))
        ep = loader.plan_epoch()
        assert len(ep) == len(loader) == 5 // world
        for j in range(len(ep)):                                          # batch j of the rank is batch rank + j * world of the epoch
            k = rank + j * world
            assert np.array_equal(ep.plan[j], full.plan[k]) and ep.sizes[j] == full.sizes[k] and ep.widths[j] == full.widths[k]
        shards.append({int(c) for j in range(len(ep)) for c in ep.plan[j, :ep.sizes[j], 0]})
    for i in range(world):
        for j in range(i + 1, world):
            assert not shards[i] & shards[j]
    assert set().union(*shards) == {int(c) for k in range(kept) for c in full.plan[k, :full.sizes[k], 0]}
    with pytest.raises(ValueError):
        Dm.ResidentMelLoader(corpus, BS, shard=(2, 2))


def test_wrapper_refusals(monkeypatch):
    """Every refusal is an error raised before anything is launched (there is no device here to launch on)."""
    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(_lib, "call", no_launch)
    corpus = torch.zeros(100, 80)
    ok = torch.tensor([[0, 10, 20], [1, 80, 20]], dtype=torch.int64)

    def plan(start, count):
        return torch.tensor([[0, 10, 20], [1, start, count]], dtype=torch.int64)

    with pytest.raises(_lib.NsgError, match="count outside"):
        ops.collate_mels(corpus, plan(0, 33), 32)                          # count > T
    with pytest.raises(_lib.NsgError, match="count outside"):
        ops.collate_mels(corpus, plan(0, -1), 32)
    with pytest.raises(_lib.NsgError, match="past the corpus"):
        ops.collate_mels(corpus, plan(81, 20), 32)                         # start + count > corpus_frames
    with pytest.raises(_lib.NsgError, match="start < 0"):
        ops.collate_mels(corpus, plan(-1, 20), 32)
    with pytest.raises(_lib.NsgError, match="plan: expected torch.int64"):
        ops.collate_mels(corpus, ok.to(torch.int32), 32)
    with pytest.raises(_lib.NsgError, match="corpus: expected a contiguous"):
        ops.collate_mels(torch.zeros(80, 100).t(), ok, 32)
    with pytest.raises(_lib.NsgError, match="corpus: expected torch.float32"):
        ops.collate_mels(corpus.double(), ok, 32)
    with pytest.raises(_lib.NsgError, match="n_mels"):
        ops.collate_mels(torch.zeros(100, 129), ok, 32)
    with pytest.raises(_lib.NsgError, match="T = 0"):
        ops.collate_mels(corpus, ok, 0)
    with pytest.raises(_lib.NsgError, match="is not .B, 3."):
        ops.collate_mels(corpus, ok[:0], 32)
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):      # a legal call, but on the host: there is no CPU path
        ops.collate_mels(corpus, ok, 32)
    # an epoch's plan with one width per batch
    ops.check_collate_plan(np.array([[[0, 0, 5]], [[0, 95, 5]]]), np.array([[5], [5]]), 100)
    with pytest.raises(_lib.NsgError, match="count outside"):
        ops.check_collate_plan(np.array([[[0, 0, 5]], [[0, 90, 6]]]), np.array([[6], [5]]), 100)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """nsg_collate_mels' own refusals (pointers that are never dereferenced): a negative status and a message."""
    import ctypes
    lib = _lib.load()
    P, OK = ctypes.c_void_p, 0x10000

    def collate(corpus=OK, frames=100, n_mels=80, plan=OK, B=2, T=64, out=OK):
        return lib.nsg_collate_mels(P(corpus), frames, n_mels, P(plan), B, T, P(out), None)

    for change in (dict(corpus=0), dict(plan=0), dict(out=0), dict(B=0), dict(B=-1), dict(T=0), dict(T=-5), dict(n_mels=0), dict(n_mels=129),
                   dict(n_mels=-80), dict(frames=-1)):
        assert collate(**change) == -1, change
        assert lib.nsg_last_error_string().startswith(b"nsg_collate_mels:"), change
