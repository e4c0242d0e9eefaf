"""GPU: the training and evaluation half of classifier-free guidance -- train_prior's label dropout (off it changes nothing, bit
for bit; at 1 the epoch is the one on null labels) for the fused step and a torch optimiser, evaluate.label_information, and
run_prior_epoch's sample_controls."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import data as Dm, evaluate as E, models as M  # noqa: E402
from neural_sound_generation_amd.epoch import run_prior_epoch  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from neural_sound_generation_amd.prior_train import PriorTrainStep, train_prior  # noqa: E402

DEV = "cuda:0"
N_CLASSES, NULL = 4, 3               # three speakers and a null class


class _Args:
    model, dataset, dim, z_dim, beta, log_interval = "pixelcnn", "arctic", 16, 32, 1.0, 1000

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Batches(list):
    """A loader's batches, materialised: every epoch of a test sees the same clips in the same order."""
    dataset = ()


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("guidance") / "arctic")
    Dm.write_synthetic_data_root(root, n_utts=12, n_speakers=3, with_audio=False, seed=3)
    loaders = Dm.get_data_loaders(root, batch_size=4, num_workers=0, frame_multiple=4, test_size=0.25)
    random.seed(7)
    np.random.seed(7)
    train = _Batches(list(loaders["train"])[:2])
    test = _Batches(loaders["test"])
    assert len(train) == 2 and all(b[3] is not None for b in train)
    torch.manual_seed(1)
    return train, test, M.VQVAE(1, 16, 32).to(DEV).eval()


def _fresh(fused):
    torch.manual_seed(4)
    prior = GatedPixelCNN(32, 16, 3, N_CLASSES).to(DEV)
    return prior, PriorTrainStep(prior, lr=3e-3) if fused else torch.optim.Adam(prior.parameters(), lr=3e-3)


def _epoch(vqvae, batches, fused, **dropout):
    prior, step = _fresh(fused)
    loss = train_prior(_Args(**dropout), vqvae, prior, step, batches, DEV, 1)
    return loss, {k: v.clone() for k, v in prior.state_dict().items()}


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(v, b[1][k]) for k, v in a[1].items())


@pytest.mark.parametrize("fused", [True, False], ids=["PriorTrainStep", "torch_optimiser"])
def test_label_dropout_in_train_prior(setup, fused):
    train, _, vqvae = setup
    base = _epoch(vqvae, train, fused)
    assert np.isfinite(base[0])
    assert _same(_epoch(vqvae, train, fused, label_dropout=0.0), base)
    assert _same(_epoch(vqvae, train, fused, label_dropout=0.0, null_label=NULL, label_dropout_seed=5), base)
    null_batches = _Batches((x, y, c, torch.full_like(g, NULL), n) for x, y, c, g, n in train)
    on_null = _epoch(vqvae, null_batches, fused)
    assert not _same(on_null, base), "the labels do not matter to this epoch: the case checks nothing"
    assert _same(_epoch(vqvae, train, fused, label_dropout=1.0, null_label=NULL), on_null)
    assert _same(_epoch(vqvae, train, fused, label_dropout=1, null_label=NULL, label_dropout_seed=9), on_null)
    # in between: the labels are the restatement's, and the same (seed, epoch) gives the same epoch
    half = _epoch(vqvae, train, fused, label_dropout=0.5, null_label=NULL, label_dropout_seed=2)
    assert _same(_epoch(vqvae, train, fused, label_dropout=0.5, null_label=NULL, label_dropout_seed=2), half)
    g = torch.Generator().manual_seed((2 << 32) | 1)
    dropped = _Batches((x, y, c, torch.where(torch.rand(len(c), generator=g) < 0.5, torch.tensor(NULL), s), n) for x, y, c, s, n in train)
    assert _same(_epoch(vqvae, dropped, fused), half)


def test_label_information(setup, capsys):
    _, test, vqvae = setup
    prior, _ = _fresh(True)
    nll = torch.zeros(2, dtype=torch.float64, device=DEV)
    count = 0
    for x, y, c, g, input_lengths in test:
        codes, lengths = E.codes_from_mels(vqvae, c.to(DEV).unsqueeze(1), input_lengths)
        a, n = prior.nll(codes, g, lengths)
        b, _ = prior.nll(codes, torch.full_like(g, NULL), lengths)
        nll[0] += a.double().sum()
        nll[1] += b.double().sum()
        count += int(n.sum())
    cond, uncond = float(nll[0]) / count, float(nll[1]) / count        # IEEE fp64 quotients (a tensor / a Python number multiplies by 1 / it)
    got = E.label_information(_Args(), vqvae, prior, test, DEV, NULL)
    assert got == {"nats_conditional": cond, "nats_unconditional": uncond, "gain": uncond - cond}
    assert cond > 0 and uncond > 0 and got["gain"] != 0.0
    assert "gain" in capsys.readouterr().out
    assert E.test_prior(_Args(), vqvae, prior, test, DEV, 0) == cond           # the conditional figure is test_prior's
    # class embeddings with equal rows: the label tells this prior nothing, exactly
    with torch.no_grad():
        for layer in prior.layers:
            w = layer.class_cond_embedding.weight
            w.copy_(w[:1].expand_as(w))
    got = E.label_information(_Args(), vqvae, prior, test, DEV, NULL)
    assert got["gain"] == 0.0 and got["nats_conditional"] == got["nats_unconditional"] > 0
    for bad in (N_CLASSES, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            E.label_information(_Args(), vqvae, prior, test, DEV, bad)
    with pytest.raises(ValueError):
        E.label_information(_Args(), vqvae, prior, _Batches(), DEV, NULL)


def test_run_prior_epoch_forwards_sample_controls(setup, tmp_path, monkeypatch):
    train, test, vqvae = setup
    monkeypatch.chdir(tmp_path)
    prior, step = _fresh(True)
    label = torch.tensor([0, 2])
    controls = dict(top_p=0.9, guidance=2.0, null_label=NULL)
    out = run_prior_epoch(_Args(sampledir=str(tmp_path / "samples")), vqvae, prior, step, train, test, DEV, 1,
                          checkpoint_path=str(tmp_path / "prior.pth.tar"), sample_label=label, sample_frames=32,
                          generator=torch.Generator(device=DEV).manual_seed(3), sample_controls=controls)
    want = prior.sample(label.to(DEV), shape=(20, 8), batch_size=2, generator=torch.Generator(device=DEV).manual_seed(3), **controls)
    assert torch.equal(out["sample_codes"], want)
    assert not torch.equal(want, prior.sample(label.to(DEV), shape=(20, 8), batch_size=2, generator=torch.Generator(device=DEV).manual_seed(3),
                                              top_p=0.9))
    assert np.load(out["samples"], allow_pickle=False).shape == (2, 80, 32)
