"""One epoch of the reference's driver loop (src/main.py:128-220, vqvae / ljspeech branch) with every stage on this
package: train_vqvae -> test_vqvae -> reconstruct the first test batch -> np.save it -> invert the last clip's mel to a
waveform (Griffin-Lim) -> save_wav -> checkpoint.  File names follow the reference's.  The CLI / argument parsing of
main.py stays out of scope; `args` is any object with the fields used below
(model, dataset, dim, z_dim, beta, log_interval, sampledir).  run_conditioned_epoch is the same loop for the speaker- and
F0-conditioned decoder's fused step (an extension).
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

from . import audio as nsg_audio
from .evaluate import (_f0_tracker, batch_conditioning, checkpoint_state, sample_mels, save_checkpoint, test_conditioned, test_prior,
                       test_vae, test_vqvae)
from .prior_train import PriorTrainStep, train_prior
from .train import train_conditioned, train_vqvae
from .vae_train import VAETrainStep, train_vae

SAMPLING_RATE, FFT_SIZE, HOP_SIZE, N_MELS = 22050, 1024, 256, 80      # src/main.py:167-170


def _averaged(optimizer, eval_with_ema):
    """The context the evaluation runs in: the optimiser's averaged weights (FlatAdam(weight_ema_decay=).ema_weights()) or
    nothing.  (Both drivers have called _require_average before they train.)"""
    return optimizer.ema_weights() if eval_with_ema else contextlib.nullcontext()


def _require_average(optimizer, eval_with_ema):
    if eval_with_ema and getattr(optimizer, "shadow", None) is None:
        raise ValueError("eval_with_ema needs an optimiser that keeps averaged weights (FlatAdam(weight_ema_decay=...))")


def run_epoch(args, model, optimizer, train_loader, test_loader, device, epoch, checkpoint_path=None, export_audio=True,
              eval_with_ema=False):
    """Returns a dict with the numbers and the files written.  eval_with_ema: the test loop and the exported reconstruction
    (nothing else) see the optimiser's averaged weights; BatchNorm running statistics are the raw model's.  The checkpoint
    always holds the raw weights, and the averaged ones inside the optimiser's state."""
    _require_average(optimizer, eval_with_ema)                         # (before an epoch is spent on training)
    train_loss = train_vqvae(args, model, optimizer, train_loader, device, epoch)
    with _averaged(optimizer, eval_with_ema):
        out = _evaluate_and_export(args, model, test_loader, device, epoch, export_audio)
    out["train_loss"] = train_loss
    out["checkpoint"] = save_checkpoint(args, checkpoint_state(epoch, args.model, model, optimizer), filename=checkpoint_path)
    return out


def _evaluate_and_export(args, model, test_loader, device, epoch, export_audio):
    loss_recons, loss_vq = test_vqvae(args, model, test_loader, device, epoch)
    out = {"test_loss_recons": loss_recons, "test_loss_vq": loss_vq}
    return _export_first_batch(args, model, test_loader, device, epoch, export_audio, out)


def _export_first_batch(args, model, test_loader, device, epoch, export_audio, out, conditioning=None):
    """Reconstruct the loader's first batch in eval mode (model(c)[0]: both autoencoders return the image first), save it as
    a .npy and, with export_audio, invert the last clip to a wav (main.py:150-187); the files' names go into `out`.
    conditioning(batch) -> (c on the device, g, f0_bins): the model is then called under them, model(c, g, f0_bins)[0]."""
    sample_dir = os.path.join(args.sampledir, format(args.dataset))
    os.makedirs(sample_dir, exist_ok=True)
    stem = '_' + str(args.model) + '_data_' + str(args.dataset) + '_dim_' + str(args.dim) + '_z_dim_' + str(args.z_dim) + '_epoch_' + str(epoch)
    with torch.no_grad():
        batch = next(iter(test_loader))
        print("Evaluating samples")
        model.eval()
        if conditioning is None:
            reconstruction = model(batch[2].to(device).unsqueeze(1))[0]   # main.py:150-153
        else:
            reconstruction = model(*conditioning(batch))[0]
        reconstruction = reconstruction.squeeze(1)
        rec_np = reconstruction.float().cpu().numpy()
        out["reconstruction"] = os.path.join(sample_dir, 'reconstruction' + stem + '.npy')
        np.save(out["reconstruction"], rec_np, allow_pickle=False)
        if export_audio:
            print("Trying audio reconstruction on test set..")
            # (the reference concatenates the batch's mels but then inverts `mel`, the last clip: main.py:166-187)
            mel = reconstruction[-1:].contiguous()
            assert mel.shape[1] == N_MELS
            signal = nsg_audio.inv_mel_spectrogram(mel, SAMPLING_RATE, FFT_SIZE, HOP_SIZE, N_MELS)[0].cpu().numpy()
            out["wav"] = os.path.join(sample_dir, 'audio_recon' + stem + '_fftsize_' + str(FFT_SIZE) + '_hopsize_' + str(HOP_SIZE) + '.wav')
            nsg_audio.save_wav(signal, out["wav"], SAMPLING_RATE)
    return out


def run_conditioned_epoch(args, model, step, train_loader, test_loader, device, epoch, checkpoint_path=None, export_audio=True,
                          eval_with_ema=False, tracker="yin", tracker_options=None, pitch_perturb=None, generator=None):
    """run_epoch for a speaker- and / or F0-conditioned VQ-VAE on its FusedTrainStep `step` (an extension): train_conditioned ->
    test_conditioned -> the first test batch reconstructed UNDER ITS OWN CONDITIONING (its g, and its bins: the sixth element of
    a data.ResidentMelLoader(f0=) batch, or tracked from its audio with tracker / tracker_options) -> the .npy, the wav and the
    checkpoint (checkpoint_state of the model and step.opt) under run_epoch's file names.  eval_with_ema as in run_epoch.
    pitch_perturb, generator: train_conditioned's (the training half only; the loaders must yield audio:
    get_data_loaders(with_audio=True) or get_resident_loaders(audio=True)); the defaults leave the loop as it was.
    Returns run_epoch's dict."""
    optimizer = step.opt
    _require_average(optimizer, eval_with_ema)
    track = _f0_tracker("run_conditioned_epoch", tracker, tracker_options)
    train_loss = train_conditioned(args, model, step, train_loader, device, epoch, tracker, tracker_options, pitch_perturb, generator)
    with _averaged(optimizer, eval_with_ema):
        loss_recons, loss_vq = test_conditioned(args, model, test_loader, device, epoch, tracker, tracker_options)
        out = _export_first_batch(args, model, test_loader, device, epoch, export_audio, {"test_loss_recons": loss_recons, "test_loss_vq": loss_vq},
                                  conditioning=lambda batch: batch_conditioning("run_conditioned_epoch", model, batch, device, track))
    out["train_loss"] = train_loss
    out["checkpoint"] = save_checkpoint(args, checkpoint_state(epoch, args.model, model, optimizer), filename=checkpoint_path)
    return out


def run_vae_epoch(args, model, step_or_optimizer, train_loader, test_loader, device, epoch, checkpoint_path=None, export_audio=True):
    """The same epoch for the continuous VAE (args.model == 'vae', the reference's default): train_vae -> test_vae ->
    reconstruction .npy -> Griffin-Lim wav of the last clip -> checkpoint ({'epoch', 'arch': 'vae', 'state_dict', 'optimizer'},
    checkpoint_filename's layout).  step_or_optimizer: a VAETrainStep (its fused step runs every batch) or a torch optimiser
    (train_vae's autograd step)."""
    if isinstance(step_or_optimizer, VAETrainStep):
        step, optimizer = step_or_optimizer, step_or_optimizer.opt
        model.train()
        total, n = torch.zeros((), device=device), 0
        for x, y, c, g, input_lengths in train_loader:
            rec, kl = step.step(c.to(device).unsqueeze(1))
            total += rec + step.kl_weight * kl
            n += 1
        if n == 0:
            raise ValueError("run_vae_epoch: empty loader")
        train_loss = float(total / n)
        print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, train_loss))
    else:
        optimizer = step_or_optimizer
        train_loss = train_vae(args, model, optimizer, train_loader, device, epoch)
    out = {"train_loss": train_loss, "test_loss": test_vae(args, model, test_loader, device, epoch)}
    _export_first_batch(args, model, test_loader, device, epoch, export_audio, out)
    out["checkpoint"] = save_checkpoint(args, checkpoint_state(epoch, 'vae', model, optimizer), filename=checkpoint_path)
    return out


def run_prior_epoch(args, vqvae, prior, step_or_optimizer, train_loader, test_loader, device, epoch, checkpoint_path=None,
                    sample_label=None, sample_frames=64, generator=None, eval_with_ema=False, sample_controls=None):
    """Stage two's epoch: train_prior -> test_prior -> checkpoint ({'epoch', 'arch': 'pixelcnn', 'state_dict', 'optimizer'}, the
    layout of run_epoch's; evaluate.load_checkpoint into the prior and the step's optimiser resumes bit-identically) -> with
    sample_label (B,) int64: evaluate.sample_mels of those classes, sample_frames frames each, saved as a .npy of mels
    (B, 80, sample_frames); sample_controls: a dict of GatedPixelCNN.sample's controls forwarded to sample_mels (temperature,
    top_k, top_p, guidance, null_label).  step_or_optimizer: a PriorTrainStep or a torch optimiser (train_prior).  The VQ-VAE is only read.
    eval_with_ema: test_prior and the samples (nothing else) see the prior's averaged weights (FlatAdam(weight_ema_decay=));
    the checkpoint always holds the raw weights, and the averaged ones inside the optimiser's state.
    Returns a dict with the numbers and the files written."""
    optimizer = step_or_optimizer.opt if isinstance(step_or_optimizer, PriorTrainStep) else step_or_optimizer
    _require_average(optimizer, eval_with_ema)
    train_loss = train_prior(args, vqvae, prior, step_or_optimizer, train_loader, device, epoch)
    with _averaged(optimizer, eval_with_ema):
        nats = test_prior(args, vqvae, prior, test_loader, device, epoch)
    out = {"train_loss": train_loss, "test_nats_per_code": nats, "test_bits_per_code": nats / float(np.log(2.0))}
    if checkpoint_path is None:
        checkpoint_path = './models/pixelcnn/checkpoint_{}_{}_{}.pth.tar'.format(args.dataset, args.dim, args.z_dim)
    out["checkpoint"] = save_checkpoint(args, checkpoint_state(epoch, 'pixelcnn', prior, optimizer), filename=checkpoint_path)
    if sample_label is not None:
        sample_dir = os.path.join(args.sampledir, format(args.dataset))
        os.makedirs(sample_dir, exist_ok=True)
        stem = '_pixelcnn_data_' + str(args.dataset) + '_dim_' + str(args.dim) + '_z_dim_' + str(args.z_dim) + '_epoch_' + str(epoch)
        was_training = vqvae.training
        vqvae.eval()
        try:
            with _averaged(optimizer, eval_with_ema):
                codes, mels = sample_mels(vqvae, prior, sample_label.to(device), sample_frames, generator=generator,
                                          **(sample_controls or {}))
        finally:
            vqvae.train(was_training)
        out["sample_codes"] = codes
        out["samples"] = os.path.join(sample_dir, 'prior_samples' + stem + '.npy')
        np.save(out["samples"], mels.squeeze(1).float().cpu().numpy(), allow_pickle=False)
    return out
