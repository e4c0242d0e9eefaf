"""CPU: the host-side pieces of the prior's training path -- length arithmetic, the label fallback, argument errors, the
masked targets -- none of which needs a GPU."""
import pytest
import torch

from neural_sound_generation_amd.evaluate import codes_from_mels, latent_lengths
from neural_sound_generation_amd.prior import GatedPixelCNN, masked_targets
from neural_sound_generation_amd.prior_train import PriorTrainStep, prior_labels


def test_latent_lengths_arithmetic():
    lens = torch.tensor([0, 255, 256, 1023, 1024, 40 * 256, 43 * 256, 44 * 256, 1000 * 256])
    got = latent_lengths(lens, 11)
    assert got.dtype == torch.int64 and got.tolist() == [0, 0, 0, 0, 1, 10, 10, 11, 11]     # (samples // 256) // 4, clipped to the grid
    assert latent_lengths(torch.tensor([1024]), 5, hop_size=128).tolist() == [2]
    with pytest.raises(ValueError):
        latent_lengths(lens, 11, hop_size=0)


def test_masked_targets():
    x = torch.arange(2 * 3 * 4).view(2, 3, 4)
    t = masked_targets(x, torch.tensor([4, 1]))
    assert torch.equal(t[0], x[0]) and torch.equal(t[1, :, :1], x[1, :, :1]) and bool((t[1, :, 1:] == -1).all())
    assert bool((masked_targets(x, torch.tensor([0, 0])) == -1).all())


def test_label_fallback_and_range():
    prior = GatedPixelCNN(32, 16, 2, 3)
    assert prior_labels(prior, None, 5).tolist() == [0] * 5 and prior_labels(prior, None, 5).dtype == torch.int64
    g = torch.tensor([0, 2, 1])
    assert prior_labels(prior, g, 3) is g
    for bad in (torch.tensor([0, 3, 1]), torch.tensor([-1, 0, 0]), torch.tensor([0, 1]), torch.tensor([0, 1, 2], dtype=torch.int32)):
        with pytest.raises(ValueError):
            prior_labels(prior, bad, 3)


def test_entry_points_refuse_bad_batches_before_the_gpu():
    """loss, nll and PriorTrainStep.forward_backward raise ValueError for a label outside [0, n_classes), a length outside
    [0, W] and malformed tensors; everything lives on the CPU here, so the checks are all that runs."""
    prior = GatedPixelCNN(32, 16, 2, 3)
    x = torch.zeros(2, 4, 5, dtype=torch.int64)
    label, lengths = torch.tensor([0, 2]), torch.tensor([5, 0])
    bad = [dict(label=torch.tensor([0, 3])), dict(label=torch.tensor([-1, 0])), dict(label=torch.tensor([0])),
           dict(label=torch.tensor([0, 1], dtype=torch.int32)), dict(lengths=torch.tensor([6, 0])), dict(lengths=torch.tensor([5, -1])),
           dict(lengths=torch.tensor([5])), dict(lengths=torch.tensor([5.0, 1.0])), dict(x=x.int()), dict(x=x[0])]
    step = PriorTrainStep.__new__(PriorTrainStep)        # the checks come first: no optimiser (and so no GPU) is needed for them
    step.model = prior
    for change in bad:
        a = dict(dict(x=x, label=label, lengths=lengths), **change)
        for fn in (prior.loss, prior.nll, step.forward_backward):
            with pytest.raises(ValueError):
                fn(a["x"], a["label"], a["lengths"])
    assert prior.check_batch(x, label, lengths)[2].tolist() == [5, 0]
    assert prior.check_batch(x, label)[2] is None


def test_codes_from_mels_checks_its_arguments():
    with pytest.raises(ValueError):
        codes_from_mels(None, torch.zeros(2, 2, 80, 8), torch.tensor([2048, 2048]))
    with pytest.raises(ValueError):
        codes_from_mels(None, torch.zeros(2, 80, 8), torch.tensor([2048]))
    with pytest.raises(ValueError):
        codes_from_mels(None, torch.zeros(2, 80, 8), torch.tensor([2048.0, 2048.0]))
