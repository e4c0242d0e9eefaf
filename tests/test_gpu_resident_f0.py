"""GPU: the resident F0 corpus -- nsg_collate_f0_bins against the composition it is defined as (a gather by the plan, then
nsg_f0_bins; torch.equal throughout) and against its numpy restatement (tests/helpers/resident_f0_ref.py); every refusal of its
contract; data.ResidentMelCorpus.track_f0 against each clip tracked alone, whatever the grouping; the loaders' six-tuples against
the five-tuples and against the host path on the frames whose windows lie inside the crop; and the consumers
(train.train_conditioned, evaluate.test_conditioned, epoch.run_conditioned_epoch) on VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).

The data roots are write_synthetic_data_root(voiced=True): tests/test_resident_f0_host.py shows, by the YIN restatement, that
such a root has voiced columns and several bins; the tests here assert the same of what they feed."""
import os
import random
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio, data as D, epoch as Ep, evaluate as E, models as M, ops  # noqa: E402
from neural_sound_generation_amd import train as T_  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep  # noqa: E402
from tests.helpers import f0_cond_ref, resident_f0_ref as R  # noqa: E402

DEV = "cuda:0"
NB, FMIN, FMAX = 8, 65.0, 500.0
F0 = {"n_bins": NB, "fmin": FMIN, "fmax": FMAX}
SPLIT = dict(test_size=0.25)                     # 8 clips: 6 train, 2 test


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the kernel against the composition -------------------------------------------------------------------------------------
FRAMES = 997


def corpus_track():
    """997 frames: unvoiced (+0.0), inside the range, below fmin, above fmax, about a quarter each."""
    rs = np.random.RandomState(3)
    kind = rs.randint(0, 4, FRAMES)
    f = np.where(kind == 0, 0.0, np.where(kind == 1, rs.uniform(FMIN, FMAX, FRAMES), np.where(kind == 2, rs.uniform(20.0, FMIN, FRAMES),
                                                                                             rs.uniform(FMAX, 900.0, FRAMES))))
    return f.astype(np.float32)


def plan_for(B, T):
    """Counts 0, 1, 3, 4, 13 and T (cut to T); starts of every residue mod 4; the last row ends on the corpus' last frame."""
    counts = [T, 0, 1, 3, 4, 13]
    plan = np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        count = min(counts[b % 6], T)
        plan[b] = (b, 20 * b + b % 4, count)
    plan[B - 1, 1] = FRAMES - plan[B - 1, 2]
    if B >= 7:
        assert sorted(set((plan[:, 1] % 4).tolist())) == [0, 1, 2, 3]
    return plan


def affine_for(B):
    rs = np.random.RandomState(B)
    return np.stack((rs.uniform(6.5, 8.0, B), rs.uniform(0.5, 1.5, B), rs.uniform(6.5, 8.0, B)), axis=1).astype(np.float32)


@pytest.mark.parametrize("with_f0", [False, True])
@pytest.mark.parametrize("with_logf", [False, True])
@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("B,T,W", [(1, 4, 1), (7, 13, 3), (9, 128, 32), (3, 64, 10)])       # (9, 128, 32): two blocks; (3, 64, 10): W < T // 4
def test_kernel_is_the_gather_then_f0_bins(B, T, W, with_affine, with_logf, with_f0):
    track, plan = corpus_track(), plan_for(B, T)
    aff = affine_for(B) if with_affine else None
    rows, count = R.gather(track, plan, T)
    assert (B * W > 256) == (B == 9)                            # one case spans more than one block of 256 columns
    td, ad = torch.from_numpy(track).to(DEV), (torch.from_numpy(aff).to(DEV) if with_affine else None)
    out = ops.collate_f0_bins(td, torch.from_numpy(plan), T, NB, FMIN, FMAX, W=W, affine=ad, want_logf=with_logf, want_f0=with_f0)
    out = list(out) if isinstance(out, tuple) else [out]
    assert len(out) == 1 + with_logf + with_f0
    bins = out.pop(0)
    logf = out.pop(0) if with_logf else None
    f0_out = out.pop(0) if with_f0 else None
    # the composition on the device: nsg_f0_bins of the gathered, padded rows with frames = count
    want_b, want_l = ops.f0_bins(torch.from_numpy(rows).to(DEV), W, NB, FMIN, FMAX, frames=count.tolist(), affine=ad, want_logf=True)
    assert bins.dtype == torch.int64 and tuple(bins.shape) == (B, W) and torch.equal(bins, want_b)
    # the numpy restatement
    ref_b, ref_l, ref_rows = R.collate_bins_f32(track, plan, T, NB, FMIN, FMAX, W=W, affine=aff)
    assert torch.equal(bins.cpu(), torch.from_numpy(ref_b))
    if with_logf:
        assert tuple(logf.shape) == (B, W) and torch.equal(bits(logf), bits(want_l))
        assert torch.equal(bits(logf).cpu(), bits(torch.from_numpy(ref_l)))
    if with_f0:
        assert tuple(f0_out.shape) == (B, T) and torch.equal(bits(f0_out).cpu(), bits(torch.from_numpy(ref_rows)))
    # the same launch on a plan that is already on the device, and the default W
    again = ops.collate_f0_bins(td, torch.from_numpy(plan).to(DEV), T, NB, FMIN, FMAX, W=W, affine=ad)
    assert torch.equal(again, bins)
    if W == T // 4:
        assert torch.equal(ops.collate_f0_bins(td, torch.from_numpy(plan), T, NB, FMIN, FMAX, affine=ad), bins)
    if B == 9 and not with_affine:
        assert len(set(ref_b.flatten().tolist())) >= 4 and (ref_b == 0).any()                # several bins and unvoiced columns


def test_a_device_plan_out_of_range_reads_zeros():
    """The kernel's clamps (nsg_collate_mels'): count into [0, T], a frame outside the corpus reads +0.0 -- every access in range."""
    track, T = corpus_track(), 16
    plan = np.array([[0, -5, 16], [1, FRAMES - 2, 13], [2, 1 << 40, 16], [3, -(1 << 40), 16], [4, 10, -3], [5, 11, T + 100],
                     [6, FRAMES, 4], [7, -16, 16], [8, (1 << 62), 16]], dtype=np.int64)
    td = torch.from_numpy(track).to(DEV)
    bins, logf, f0_out = ops.collate_f0_bins(td, torch.from_numpy(plan).to(DEV), T, NB, FMIN, FMAX, want_logf=True, want_f0=True)
    ref_b, ref_l, ref_rows = R.collate_bins_f32(track, plan, T, NB, FMIN, FMAX)
    torch.cuda.synchronize()
    assert torch.equal(bins.cpu(), torch.from_numpy(ref_b)) and torch.equal(bits(logf).cpu(), bits(torch.from_numpy(ref_l)))
    assert torch.equal(bits(f0_out).cpu(), bits(torch.from_numpy(ref_rows)))
    assert ref_rows[0, :5].tolist() == [0.0] * 5 and np.array_equal(ref_rows[0, 5:], track[:11])
    assert np.array_equal(ref_rows[1, :2], track[-2:]) and not ref_rows[1, 2:].any()
    assert not ref_rows[[2, 3, 4, 6, 7, 8]].any() and np.array_equal(ref_rows[5], track[11:27])
    with pytest.raises(_lib.NsgError, match="collate plan"):                                  # the same plan on the host is refused
        ops.collate_f0_bins(td, torch.from_numpy(plan), T, NB, FMIN, FMAX)


def test_every_refusal_leaves_the_outputs_untouched():
    B, T, W = 4, 26, 6
    td = torch.from_numpy(corpus_track()).to(DEV)
    plan = torch.from_numpy(plan_for(B, T)).to(DEV)
    aff = torch.from_numpy(affine_for(B)).to(DEV)
    bins = torch.full((B, W), -7, dtype=torch.int64, device=DEV)
    logf = torch.full((B, W), -7.0, device=DEV)
    f0_out = torch.full((B, T), -7.0, device=DEV)
    p = lambda t, off=0: c_void_p(t.data_ptr() + off)                                           # noqa: E731
    null = c_void_p(0)
    base = dict(corpus=p(td), frames=FRAMES, plan=p(plan), affine=p(aff), bins=p(bins), logf=p(logf), f0_out=p(f0_out), B=B, T=T, W=W, n_bins=NB,
                fmin=FMIN, fmax=FMAX)
    same = [(float(f), float(np.nextafter(f, np.float32(1e3)))) for f in np.arange(100, 120, dtype=np.float32)]
    below, above = next((f, g) for f, g in same if np.float32(np.log2(f)) == np.float32(np.log2(g)))
    nan, inf = float("nan"), float("inf")
    bad = [dict(corpus=null), dict(plan=null), dict(bins=null),
           dict(B=0), dict(T=0), dict(W=0), dict(B=-1), dict(T=-26), dict(W=-6),
           dict(W=7), dict(T=23),
           dict(n_bins=0), dict(n_bins=-1),
           dict(fmin=0.0), dict(fmin=-65.0), dict(fmin=500.0), dict(fmin=600.0), dict(fmin=nan), dict(fmax=nan), dict(fmax=inf),
           dict(fmin=below, fmax=above),
           dict(frames=-1),
           dict(corpus=p(td, 2)), dict(affine=p(aff, 2)), dict(logf=p(logf, 2)), dict(f0_out=p(f0_out, 2)), dict(plan=p(plan, 4)), dict(bins=p(bins, 4)),
           dict(B=1 << 16, T=1 << 15, W=8)]
    for kw in bad:
        a = dict(base, **kw)
        with pytest.raises(_lib.NsgError, match="nsg_collate_f0_bins"):
            _lib.call("nsg_collate_f0_bins", a["corpus"], a["frames"], a["plan"], a["affine"], a["bins"], a["logf"], a["f0_out"], a["B"], a["T"],
                      a["W"], a["n_bins"], a["fmin"], a["fmax"], ops._stream())
    torch.cuda.synchronize()
    assert bool((bins == -7).all()) and bool((logf == -7.0).all()) and bool((f0_out == -7.0).all())
    # (the unchanged arguments are served)
    a = base
    _lib.call("nsg_collate_f0_bins", a["corpus"], a["frames"], a["plan"], a["affine"], a["bins"], a["logf"], a["f0_out"], a["B"], a["T"], a["W"],
              a["n_bins"], a["fmin"], a["fmax"], ops._stream())
    assert not bool((bins == -7).any()) and not bool((logf == -7.0).any()) and not bool((f0_out == -7.0).any())


# ---- the corpus -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    """8 voiced clips of 40 .. 90 frames, two speakers; the train split holds 6 of them, of both speakers, two longer than 64 frames."""
    path = str(tmp_path_factory.mktemp("resident_f0") / "root")
    D.write_synthetic_data_root(path, n_utts=8, min_frames=40, max_frames=90, n_speakers=2, seed=11, voiced=True)
    return path


def sources(root, train=True):
    kw = dict(train=train, **SPLIT)
    return D.MelSpecDataSource(root, **kw), D.RawAudioDataSource(root, **kw)


def tracked(root, train=True, **kw):
    mel, wav = sources(root, train)
    return D.ResidentMelCorpus(mel, DEV).track_f0(wav, **kw)


@pytest.fixture(scope="module")
def corpus(root):
    return tracked(root)


@pytest.fixture(scope="module")
def clips(root):
    """The train split's waveforms (numpy), read once."""
    _, wav = sources(root)
    return [np.load(p) for p in wav.paths]


@pytest.mark.parametrize("tracker", ["yin", "viterbi"])
def test_corpus_track_is_each_clip_tracked_alone(root, corpus, clips, tracker):
    c = corpus if tracker == "yin" else tracked(root, tracker="viterbi")
    alone = audio.f0 if tracker == "yin" else audio.f0_track
    assert len(c) == 6 and c.n_frames.min() >= 40 and c.n_frames.max() <= 90 and (c.n_frames > 64).sum() >= 2
    assert c.f0.dtype == torch.float32 and tuple(c.f0.shape) == (int(c.offsets[-1]),) and c.f0.device == c.frames.device
    assert c.f0_settings == {"tracker": tracker, "tracker_options": {}, "fmin": 65.0, "fmax": 500.0}
    for i, wav in enumerate(clips):
        nf = int(c.n_frames[i])
        f0, _ = alone(torch.from_numpy(wav).unsqueeze(0).to(DEV))
        assert f0.shape[1] == nf + 1
        got = c.f0[int(c.offsets[i]):int(c.offsets[i + 1])]
        assert torch.equal(bits(got), bits(f0[0, :nf])), i
        # the clip's moments: audio.logf0_sums of its kept frames, and the fp64 restatement of them
        assert np.array_equal(c.f0_sums[i], audio.logf0_sums(f0[:, :nf].contiguous())[0].cpu().numpy())
        ref = f0_cond_ref.logf0_sums_f64(f0[:, :nf].cpu().numpy())[0]
        assert c.f0_sums[i, 0] == ref[0] and np.allclose(c.f0_sums[i, 1:], ref[1:], rtol=1e-12, atol=0)
    assert c.f0_sums.dtype == np.float64 and c.f0_sums.shape == (6, 3)
    assert 2 * int((c.f0 > 0).sum()) >= c.f0.numel()                                            # at least half of all frames are voiced


def test_corpus_does_not_depend_on_the_grouping(root, corpus):
    one = tracked(root, group_clips=1)
    many = tracked(root, group_clips=64)
    split = tracked(root, group_samples=40000)                  # clips of 10 240 .. 23 040 samples: groups of one to three
    for other in (one, many, split):
        assert torch.equal(bits(other.f0), bits(corpus.f0)) and np.array_equal(other.f0_sums, corpus.f0_sums)


def test_audio_and_mel_lengths_must_agree(root, tmp_path):
    import shutil
    broken = str(tmp_path / "broken")
    shutil.copytree(root, broken)
    _, wav = sources(broken)
    x = np.load(wav.paths[2])
    np.save(wav.paths[2], x[:-256], allow_pickle=False)
    mel, wav = sources(broken)
    c = D.ResidentMelCorpus(mel, DEV)
    with pytest.raises(ValueError, match="audio and mel lengths disagree"):
        c.track_f0(wav)
    assert c.f0 is None and c.f0_sums is None


def test_speaker_statistics_from_the_corpus(corpus, clips):
    g = corpus.speaker_ids.cpu()
    assert sorted(set(g.tolist())) == [0, 1]

    def batch(ids):
        L = max(len(clips[i]) for i in ids)
        wav = np.zeros((len(ids), L), dtype=np.float32)
        for j, i in enumerate(ids):
            wav[j, :len(clips[i])] = clips[i]
        return torch.from_numpy(wav), np.array([len(clips[i]) for i in ids]), g[ids]
    want, want_n = E.speaker_f0_stats([batch([0, 1, 2]), batch([3, 4, 5])], 2, DEV)
    got, got_n = corpus.speaker_f0_stats(2)
    assert got.dtype == torch.float64 and got_n.dtype == torch.int64 and tuple(got.shape) == (2, 2)
    assert torch.equal(got_n, want_n) and int(got_n.min()) > 50
    # fp64 sums of a few hundred terms of magnitude ~ 7 (and ~ 50 for the squares) in another order
    assert torch.allclose(got[:, 0], want[:, 0], rtol=1e-12, atol=0)
    assert torch.allclose(got[:, 1], want[:, 1], rtol=0, atol=1e-9)
    wide, wide_n = corpus.speaker_f0_stats(3)                    # a speaker without a clip: NaN and 0
    assert torch.equal(wide[:2], got) and bool(torch.isnan(wide[2]).all()) and wide_n.tolist() == got_n.tolist() + [0]


# ---- the loaders ------------------------------------------------------------------------------------------------------------
MAX_STEPS = 64 * 256


def seeded(seed):
    random.seed(seed)
    np.random.seed(seed)


def resident(root, batch_size, f0=F0, max_time_steps=MAX_STEPS):
    return D.get_resident_loaders(root, batch_size, max_time_steps=max_time_steps, frame_multiple=4, device=DEV, f0=f0, **SPLIT)


@pytest.fixture(scope="module")
def loaders(root):
    return resident(root, 2), resident(root, 2, f0=None)


@pytest.mark.parametrize("phase", ["train", "test"])
def test_loader_adds_the_bins_and_changes_nothing_else(loaders, phase):
    with_f0, plain = loaders[0][phase], loaders[1][phase]
    assert with_f0.f0 == (NB, FMIN, FMAX) and plain.f0 is None and with_f0.dataset.f0 is not None and plain.dataset.f0 is None
    seeded(5)
    six = list(with_f0)
    after = (random.random(), np.random.rand())
    seeded(5)
    five = list(plain)
    assert (random.random(), np.random.rand()) == after                                          # the same draws
    seeded(5)
    ep = with_f0.plan_epoch()
    assert len(six) == len(five) == len(ep) == (3 if phase == "train" else 1)
    for k, (a, b) in enumerate(zip(six, five)):
        assert len(a) == 6 and len(b) == 5 and a[0] is None and a[1] is None
        assert torch.equal(bits(a[2]), bits(b[2])) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
        rows, T = ep.plan[k, :int(ep.sizes[k])], int(ep.widths[k])
        assert T == a[2].shape[2] and T % 4 == 0
        want = ops.collate_f0_bins(with_f0.dataset.f0, torch.from_numpy(rows), T, NB, FMIN, FMAX)
        assert a[5].dtype == torch.int64 and a[5].is_cuda and tuple(a[5].shape) == (len(rows), T // 4) and torch.equal(a[5], want)


def test_a_batch_narrower_than_a_column_has_empty_bins(corpus):
    class Short:                                                 # the corpus with every clip cut to its first 3 frames
        f0, frames, speaker_ids, device, lengths = corpus.f0, corpus.frames, corpus.speaker_ids, corpus.device, corpus.lengths
        offsets, n_frames = corpus.offsets, np.full(6, 3, dtype=np.int64)

        def __len__(self):
            return 6
    batches = list(D.ResidentMelLoader(Short(), 4, train=False, f0=(NB, FMIN, FMAX)))
    assert [tuple(b[5].shape) for b in batches] == [(4, 0), (2, 0)] and all(b[5].dtype == torch.int64 and b[5].is_cuda for b in batches)
    assert [tuple(b[2].shape) for b in batches] == [(4, 80, 3), (2, 80, 3)]


def test_bins_are_the_host_path_s_where_the_window_lies_inside_the_crop(root, loaders):
    """The host path tracks the cropped audio (zero outside the crop), the resident path crops the whole clip's track: equal, bit
    for bit, on the frames whose YIN window (t 256 - 512 .. t 256 + 511 + tau_max) lies inside the crop, and not elsewhere."""
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=NB)
    host = D.get_data_loaders(root, 2, max_time_steps=MAX_STEPS, num_workers=0, with_audio=True, frame_multiple=4, pin_memory=False, **SPLIT)
    tau_max = audio.f0_lags(22050, 65.0, 500.0)[1]
    edge_differs = cropped = 0
    for phase in ("train", "test"):
        seeded(9)
        hb = list(host[phase])
        seeded(9)
        ep = loaders[0][phase].plan_epoch()
        seeded(9)
        rb = list(loaders[0][phase])
        assert len(hb) == len(rb) > 0
        for k, (h, r) in enumerate(zip(hb, rb)):
            assert torch.equal(h[2].to(DEV), r[2]) and torch.equal(h[4], r[4])              # the same crops
            _, _, host_bins = E.batch_conditioning("test", model, h, DEV, audio.f0)
            T = h[2].shape[2]
            count = (h[4].numpy() // 256)
            host_f0, _ = audio.f0(h[0].squeeze(1).to(DEV).contiguous(), lengths=h[4].numpy())
            rows = torch.from_numpy(ep.plan[k, :len(count)])
            res_bins, res_f0 = ops.collate_f0_bins(loaders[0][phase].dataset.f0, rows, T, NB, FMIN, FMAX, want_f0=True)
            assert torch.equal(res_bins, r[5])
            inside = np.zeros((len(count), T), dtype=bool)
            for b, n in enumerate(count):
                inside[b, :n] = R.interior(n, tau_max=tau_max)
                assert inside[b, 2:n - 3].all() and not inside[b, :2].any() and not inside[b, n - 3:].any()      # frames 2 .. count - 4
            valid = np.arange(T)[None, :] < count[:, None]
            hf, rf = host_f0[:, :T].cpu().numpy(), res_f0.cpu().numpy()
            assert np.array_equal(hf.view(np.int32)[inside], rf.view(np.int32)[inside])
            edge_differs += int((hf != rf)[valid & ~inside].sum())
            cropped += int((ep.plan[k, :len(count), 1] != loaders[0][phase].dataset.offsets[ep.plan[k, :len(count), 0]]).sum())
            cols_in, cols_valid = inside.reshape(len(count), T // 4, 4).all(-1), valid.reshape(len(count), T // 4, 4).all(-1)
            assert 2 * cols_in.sum() >= cols_valid.sum() > 0
            hbn, rbn = host_bins.cpu().numpy(), r[5].cpu().numpy()
            assert np.array_equal(hbn[cols_in], rbn[cols_in]) and len(set(rbn[cols_in].tolist()) - {0}) >= 1
    assert cropped >= 1 and edge_differs >= 1


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


def test_train_conditioned_over_the_resident_loader(root):
    seeded(3)
    batches = Fixed(resident(root, 3)["train"])
    assert len(batches) == 2 and all(len(b) == 6 and b[0] is None for b in batches)
    fed_bins = torch.cat([b[5].flatten() for b in batches])
    used = sorted(set(fed_bins.tolist()) - {0})
    assert len(used) >= 3 and 2 * int((fed_bins > 0).sum()) >= fed_bins.numel()
    model, step = fresh()
    before = model.f0_embedding.weight.detach().clone()
    losses, real = [], step.step
    step.step = lambda c, g=None, f0_bins=None: (losses.append(real(c, g, f0_bins=f0_bins)), losses[-1])[1]
    last = T_.train_conditioned(Args(), model, step, batches, DEV, 0)
    # by hand, from a second identically seeded model
    model2, step2 = fresh()
    want = [step2.step(c.unsqueeze(1), g, f0_bins=bins) for _, _, c, g, _, bins in batches]
    assert len(losses) == 2 and last == float(losses[-1][0] + losses[-1][1])
    for a, b in zip(losses, want):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    changed = (model.f0_embedding.weight.detach() != before).any(1).cpu()
    assert bool(changed[used].all()) and bool(changed[0])
    absent = sorted(set(range(NB + 1)) - set(fed_bins.tolist()))
    assert absent and not bool(changed[absent].any())                                           # a bin nobody fed keeps its row


@pytest.fixture(scope="module")
def root48(tmp_path_factory):
    """8 voiced clips of 48 frames each: with frame_multiple = 4 and no max_time_steps every crop is a whole clip."""
    path = str(tmp_path_factory.mktemp("resident_f0") / "root48")
    D.write_synthetic_data_root(path, n_utts=8, min_frames=48, max_frames=48, n_speakers=2, seed=4, voiced=True)
    return path


def test_test_conditioned(root48):
    six = Fixed(resident(root48, 1, max_time_steps=None)["test"])
    five = Fixed(D.get_data_loaders(root48, 1, num_workers=0, with_audio=True, frame_multiple=4, pin_memory=False, **SPLIT)["test"])
    assert len(six) == len(five) == 2 and all(len(b) == 6 for b in six) and all(len(b) == 5 and b[0] is not None for b in five)
    assert any(int(b[5].max()) > 0 for b in six)
    model, _ = fresh(2)
    assert float(model.f0_embedding.weight.detach().abs().min()) > 0 and float(model.speaker_embedding.weight.detach().abs().max()) > 0
    state = {k: v.clone() for k, v in model.state_dict().items()}
    got = E.test_conditioned(Args(), model, six, DEV, 0)
    assert model.training and all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    # by hand
    model.eval()
    lr_, lv = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    with torch.no_grad():
        for _, _, c, g, _, bins in six:
            c = c.unsqueeze(1)
            x_tilde, z_e, z_q = model(c, g, bins)
            lr_ += torch.nn.functional.mse_loss(torch.nn.functional.pad(x_tilde, (0, c.shape[3] - x_tilde.shape[3])), c)
            lv += torch.nn.functional.mse_loss(z_q, z_e)
    model.train()
    assert got == (float(lr_ / 2), float(lv / 2))
    # whole clips: the bins tracked from the batch's audio are the resident ones, and so is the figure
    for a, b in zip(six, five):
        assert torch.equal(a[2], b[2].to(DEV)) and torch.equal(E.batch_conditioning("test", model, b, DEV, audio.f0)[2], a[5])
    assert E.test_conditioned(Args(), model, five, DEV, 0) == got
    # test_vqvae calls model(c): no speaker row, no F0 row
    plain = E.test_vqvae(Args(), model, five, DEV, 0)
    model.train()
    assert plain[0] != got[0] and plain[1] == got[1]                                            # (the encoder and the codes do not see the conditioning)


def test_run_conditioned_epoch_writes_and_resumes(root, tmp_path):
    args = Args()
    args.sampledir = str(tmp_path / "samples")
    seeded(4)
    ld = resident(root, 3, max_time_steps=None)
    model, step = fresh(5)
    ckpt = str(tmp_path / "models" / "ckpt.pth.tar")
    out = Ep.run_conditioned_epoch(args, model, step, ld["train"], ld["test"], DEV, 1, checkpoint_path=ckpt)
    assert set(out) == {"train_loss", "test_loss_recons", "test_loss_vq", "reconstruction", "wav", "checkpoint"}
    assert all(os.path.exists(out[k]) for k in ("reconstruction", "wav", "checkpoint")) and out["checkpoint"] == ckpt
    assert os.path.basename(out["reconstruction"]) == "reconstruction_vqvae_data_synth_dim_16_z_dim_32_epoch_1.npy"
    assert os.path.basename(out["wav"]) == "audio_recon_vqvae_data_synth_dim_16_z_dim_32_epoch_1_fftsize_1024_hopsize_256.wav"
    assert np.isfinite([out["train_loss"], out["test_loss_recons"], out["test_loss_vq"]]).all() and step.opt.step_count == 2
    # the reconstruction is the first test batch under its own conditioning
    _, _, c, g, _, bins = next(iter(ld["test"]))
    model.eval()
    with torch.no_grad():
        want = model(c.unsqueeze(1), g, bins)[0].squeeze(1)
        other = model(c.unsqueeze(1))[0].squeeze(1)
    rec = np.load(out["reconstruction"], allow_pickle=False)
    assert int(bins.max()) > 0 and np.array_equal(rec, want.cpu().numpy()) and not np.array_equal(rec, other.cpu().numpy())
    # resume: the checkpoint into a fresh model and step, then the next step is bitwise the original's
    model2, step2 = fresh(6)
    st = E.load_checkpoint(ckpt, model2, step2.opt, map_location=DEV)
    assert st["epoch"] == 1 and st["arch"] == "vqvae" and step2.opt.step_count == 2
    model.train()
    a = step.step(c.unsqueeze(1), g, f0_bins=bins)
    b = step2.step(c.unsqueeze(1), g, f0_bins=bins)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    for (k, x), (_, y) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(x, y), k
    for name in ("flat_param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(step.opt, name), getattr(step2.opt, name)), name
