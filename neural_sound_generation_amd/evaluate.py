"""The step on the far side of training: evaluation-mode loss, reconstruction dump and the
checkpoint layout, restated from the reference's src/test.py:73-106 and src/main.py:61-66,137-163,216-220.

  * `test_vqvae(args, model, test_loader, device, epoch)` -- same signature and behaviour as the reference's function
    (ljspeech branch): model.eval(), forward, zero-pad the reconstruction to the input width, accumulate
    mse(target, c) and mse(z_q, z_e) over the batches, divide by the number of batches, print their sum.
    Returns (loss_recons, loss_vq) as floats (the reference returns nothing).
  * `test_vae(args, model, test_loader, device, epoch)` -- the continuous VAE's test loop (src/test.py:32-49).
  * `eval_losses(model, c)` -- the same two numbers for one batch with no autograd and no host round trip: the
    HIP forward stacks and the fused loss kernels (nsg_mse_padded folds the zero-pad).
  * `export_reconstruction(model, c, path)` -- main.py:150-163: x_tilde.squeeze(1) as a float32 .npy of shape (B, 80, T').
  * `checkpoint_state` / `save_checkpoint` / `load_checkpoint` -- main.py:61-66,216-220: {'epoch', 'arch',
    'state_dict', 'optimizer'}; state_dict keys are the reference's, the optimiser state is in torch.optim.Adam's
    layout (FlatAdam.state_dict), so checkpoints move both ways between the reference and this package.
  * `sample_mels(vqvae, prior, label, frames)` -- generation's code -> mel half: codes drawn from the latent prior
    (GatedPixelCNN.sample) on the VQ-VAE's (20, frames / 4) latent grid, decoded to mels (audio.py goes on to waveforms).
  * `codes_from_mels(vqvae, c, input_lengths)` -- stage two's input: a padded mel batch -> its codes and the number of valid
    latent columns of each clip; `test_prior(args, vqvae, prior, test_loader, device, epoch)` -- the prior's test figure, nats
    per code over the whole loader, weighted by codes (prior_train.py has the training side).
  * `continue_mels(vqvae, prior, mel, label, keep_frames, frames)` -- the same with the first keep_frames of a given mel held:
    encode, keep the leading latent columns, sample the rest (GatedPixelCNN.continue_codes), decode.
  * `continue_audio(vqvae, prior, wav, label, keep_frames, frames)` -- wav in, wav out: audio.melspectrogram, continue_mels,
    audio.inv_mel_spectrogram.
  * `convert_voice(vqvae, mel, g_target)` -- what the speaker-conditioned decoder is for: encode, decode under another speaker's
    id; `test_conversion(args, vqvae, pair_loader, device, epoch)` -- its figure over parallel utterances: the mel-cepstral
    distortion after dynamic time warping (audio.mel_cepstral_distortion) of converted against target, and of source against
    target for context; `test_conversion_f0(args, vqvae, pair_loader, device, epoch)` -- the same pairs as waveforms, judged by
    pitch: the converted mel inverted to a waveform, F0 by YIN (audio.f0), and along the same warping paths the F0 error in
    cents, the voiced / unvoiced disagreement and the log-F0 correlation (audio.f0_figures), pooled over all clips.  A model with an
    F0 table (VQVAE(n_f0_bins=)) takes the pitch as an input: `convert_voice(..., f0_bins=)`, `test_conversion_f0(..., f0_stats=)`
    feed the source's contour moved to the target speaker's log-F0 statistics; `speaker_f0_stats(wav_loader, n_speakers, device)`
    pools those statistics per speaker.
  * `test_reconstruction_audio(args, vqvae, wav_loader, device, epoch)` -- the reconstruction judged as audio against the
    recording: wav -> mel -> model -> waveform, and the mel inverted without the model beside it, each scored by STOI and ESTOI
    (audio.stoi) against the wav it came from.
  * `test_conditioned(args, model, test_loader, device, epoch)` -- test_vqvae with the model under each batch's own speaker and F0
    conditioning (bins from a resident loader's six-tuples, or tracked from the batch's audio); `batch_conditioning` is the rule
    it shares with train.train_conditioned.
  * `codebook_usage(model, loader, device)` -- how much of the codebook a dataset uses: per-code counts and their perplexity.
"""
from __future__ import annotations

import functools
import numbers
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import engine, functional as Fn, ops


@torch.no_grad()
def eval_losses(model, c: torch.Tensor):
    """c (B,1,80,T) on the GPU -> (loss_recons, loss_vq) device scalars, eval-mode statistics (running mean / var)."""
    x = Fn.to_nhwc(c)
    B, H, T, _ = x.shape
    dtype = getattr(model, "compute_dtype", torch.float32)
    encP, decP = engine.encoder_params(model.encoder), engine.decoder_params(model.decoder)
    ze, _ = engine.encoder_forward(x, encP, False, dtype=dtype)
    D = ze.shape[-1]
    cb = model.codebook.embedding.weight.detach()
    _, zq, _ = ops.vq_forward(ze.view(-1, D), cb, want_codes=True, impl=getattr(model.codebook, "search_impl", "mfma"))
    zq = zq.view_as(ze)
    xt, _ = engine.decoder_forward(zq, decP, False, dtype=dtype)
    loss_recons, _ = ops.mse_padded(xt, x, B * H, xt.shape[2], T, want_grad=False)
    loss_vq, _, _ = ops.vq_losses(ze, zq, want_dz=False, want_dq=False)
    return loss_recons[0], loss_vq[0]


def test_vqvae(args, model, test_loader, device, epoch):
    """Drop-in for src/test.py:73-106 (ljspeech branch): `test_loader` yields (x, y, c, g, input_lengths), c (B, 80, T)."""
    model.eval()
    loss_recons = torch.zeros((), device=device)
    loss_vq = torch.zeros((), device=device)
    n = 0
    with torch.no_grad():
        for step, (x, y, c, g, input_lengths) in enumerate(test_loader):
            c = c.to(device).unsqueeze(1)
            x_tilde, z_e_x, z_q_x = model(c)
            target = F.pad(x_tilde, (0, c.size(3) - x_tilde.size(3))) if x_tilde.size(3) != c.size(3) else x_tilde
            loss_recons += F.mse_loss(target, c)
            loss_vq += F.mse_loss(z_q_x, z_e_x)
            n += 1
    if n == 0:
        raise ValueError("test_vqvae: empty loader")
    loss_recons, loss_vq = float(loss_recons / n), float(loss_vq / n)
    print('====> Test set loss: {:.4f}'.format(loss_recons + loss_vq))
    return loss_recons, loss_vq


def test_vae(args, model, test_loader, device, epoch):
    """Drop-in for src/test.py:32-49 (ljspeech branch) for the continuous VAE: model.eval() (running BatchNorm statistics; the
    latent is still sampled, as there), forward, vae_train.vae_loss.  Returns the mean over the batches (the reference divides
    a sum of batch losses by the dataset size and returns nothing)."""
    from .vae_train import vae_loss
    model.eval()
    loss = torch.zeros((), device=device)
    n = 0
    with torch.no_grad():
        for step, (x, y, c, g, input_lengths) in enumerate(test_loader):
            c = c.to(device).unsqueeze(1)
            x_tilde, kl_d = model(c)
            loss += vae_loss(x_tilde, c, kl_d)
            n += 1
    if n == 0:
        raise ValueError("test_vae: empty loader")
    loss = float(loss / n)
    print('====> Test set loss: {:.4f}'.format(loss))
    return loss


@torch.no_grad()
def codebook_usage(model, loader, device):
    """Per-code usage of `model`'s codebook over a dataset: `loader` yields (x, y, c, g, input_lengths) with c (B, 80, T) mels, as
    for test_vqvae.  Returns (counts (K,) int64 on `device`: latent positions assigned to each code; perplexity: exp of the
    entropy of counts / counts.sum(), a float).  Built from model.encode (eval mode; the model's mode is restored) and
    ops.code_usage, whose int32 window is folded into the int64 counts after every batch."""
    K = model.codebook.embedding.weight.shape[0]
    counts = torch.zeros(K, dtype=torch.int64, device=device)
    window = torch.zeros(K, dtype=torch.int32, device=device)
    was_training = model.training
    model.eval()
    try:
        for x, y, c, g, input_lengths in loader:
            idx = model.encode(c.to(device).unsqueeze(1))
            ops.code_usage(idx.reshape(-1).contiguous(), K, window)
            counts += window
            window.zero_()
    finally:
        model.train(was_training)
    total = counts.sum()
    if int(total) == 0:
        raise ValueError("codebook_usage: empty loader")
    p = counts.double() / total
    nz = p > 0
    return counts, float(torch.exp(-(p[nz] * p[nz].log()).sum()))


__test__ = False  # (not a pytest module even though a function is named test_*)


@torch.no_grad()
def export_reconstruction(model, c: torch.Tensor, path: str) -> np.ndarray:
    """main.py:150-163: reconstruction of one batch as a float32 array (B, 80, T') saved with np.save."""
    was_training = model.training
    model.eval()
    x_tilde, _, _ = model(c)
    model.train(was_training)
    rec = x_tilde.squeeze(1).float().cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, rec, allow_pickle=False)
    return rec


def checkpoint_state(epoch: int, arch: str, model, optimizer) -> dict:
    return {"epoch": epoch, "arch": arch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}


def checkpoint_filename(args) -> str:
    """main.py:61-65 (the reference never creates the directory; save_checkpoint here does)."""
    return './models/{}/checkpoint_{}_{}_{}.pth.tar'.format(args.model, args.dataset, args.dim, args.z_dim)


def save_checkpoint(args, state, filename: str | None = None) -> str:
    filename = filename or checkpoint_filename(args)
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    torch.save(state, filename)
    return filename


def load_checkpoint(filename: str, model, optimizer=None, map_location=None) -> dict:
    """Loads a checkpoint written by this package or by the reference's main.py (tensors only: weights_only=True)."""
    state = torch.load(filename, map_location=map_location, weights_only=True)
    model.load_state_dict(state["state_dict"])
    if optimizer is not None and state.get("optimizer") is not None:
        optimizer.load_state_dict(state["optimizer"])
    return state


LATENT_ROWS = 20   # the VQ-VAE's latent grid of an 80-band mel: two stride-2 convolutions, 80 / 4 rows


@torch.no_grad()
def sample_mels(vqvae, prior, label: torch.Tensor, frames: int, g=None, generator=None, **controls):
    """Codes (B, 20, frames // 4) sampled from the prior for the class labels (B,), and their decoded mels (B, 1, 80, frames)
    (vqvae.decode; put the VQ-VAE in eval mode for its running BatchNorm statistics).  controls: GatedPixelCNN.sample's
    temperature, top_k and top_p.  guidance= and null_label= (classifier-free guidance) pass through to it as well."""
    if frames < 4:
        raise ValueError("sample_mels: frames must be at least 4 (one latent column)")
    codes = prior.sample(label, shape=(LATENT_ROWS, frames // 4), batch_size=label.shape[0], generator=generator, **controls)
    return codes, vqvae.decode(codes, g)


@torch.no_grad()
def codes_from_mels(vqvae, c: torch.Tensor, input_lengths: torch.Tensor, hop_size: int = 256):
    """c (B, 1, 80, T) (or (B, 80, T)) mels on the GPU, zero-padded to the batch's longest clip, T a multiple of 4;
    input_lengths (B,) int64 audio samples per clip (what the loaders yield) -> (codes (B, 20, T // 4) int64 on c's device,
    lengths (B,) int64 on input_lengths' device): lengths = (input_lengths // hop_size) // 4, clipped to the grid's width, is the
    number of latent columns that come from the clip itself.  The VQ-VAE runs in eval mode (its mode is restored) and is not
    changed.  The codes under the padding are whatever the VQ-VAE makes of zero mel; they are left out of the prior's loss
    (GatedPixelCNN.loss(..., lengths)) but still lie in the causal context of valid positions of later rows -- the vertical
    stacks reach +-3 columns in layer 0 and +-1 per later layer -- so a clip's likelihood depends slightly on how far its
    batch was padded.  That is the loader's padding showing through; nothing here hides it."""
    if c.dim() == 3:
        c = c.unsqueeze(1)
    if c.dim() != 4 or c.shape[1] != 1:
        raise ValueError("codes_from_mels: c must be (B, 1, 80, T) or (B, 80, T)")
    B = c.shape[0]
    if not isinstance(input_lengths, torch.Tensor) or tuple(input_lengths.shape) != (B,) or input_lengths.dtype != torch.int64:
        raise ValueError(f"codes_from_mels: input_lengths must be an int64 tensor of shape ({B},)")
    was_training = vqvae.training
    vqvae.eval()
    try:
        codes = vqvae.encode(c).contiguous()
    finally:
        vqvae.train(was_training)
    return codes, latent_lengths(input_lengths, codes.shape[-1], hop_size)


def latent_lengths(input_lengths: torch.Tensor, width: int, hop_size: int = 256) -> torch.Tensor:
    """(input_lengths // hop_size) // 4 clipped to [0, width]: frames per clip -> valid latent columns (two stride-2 convs)."""
    if int(hop_size) < 1:
        raise ValueError("hop_size must be positive")
    return ((input_lengths // int(hop_size)) // 4).clamp(0, int(width))


def test_prior(args, vqvae, prior, test_loader, device, epoch):
    """The prior's test figure: nats per code = sum of the clips' negative log-likelihoods / number of valid codes, over the
    whole loader (weighted by codes, not a mean of batch means); printed also as bits per code."""
    from .prior_train import prior_labels
    nll = torch.zeros((), dtype=torch.float64, device=device)
    count = torch.zeros((), dtype=torch.int64, device=device)
    n = 0
    for x, y, c, g, input_lengths in test_loader:
        c = c.to(device).unsqueeze(1)
        codes, lengths = codes_from_mels(vqvae, c, input_lengths)
        clip_nll, clip_count = prior.nll(codes, prior_labels(prior, g, len(c)), lengths)
        nll += clip_nll.double().sum()
        count += clip_count.sum()
        n += 1
    if n == 0:
        raise ValueError("test_prior: empty loader")
    if int(count) == 0:
        raise ValueError("test_prior: no clip of the loader is long enough for one latent column")
    nats = float(nll / count)
    print('====> Prior test set: {:.4f} nats per code ({:.4f} bits)'.format(nats, nats / float(np.log(2.0))))
    return nats


def label_information(args, vqvae, prior, test_loader, device, null_label):
    """How much the label tells the prior, the quantity classifier-free guidance extrapolates: one pass over the loader, each
    batch scored twice by prior.nll, under its own labels and under null_label for every clip, pooled over codes as test_prior
    pools.  Returns {"nats_conditional", "nats_unconditional", "gain"}, gain = unconditional - conditional in nats per code.
    Roughly zero for a prior trained without label dropout on a null class it never saw as such."""
    from .prior_train import prior_labels
    n_classes = prior.layers[0].class_cond_embedding.num_embeddings
    if isinstance(null_label, bool) or not isinstance(null_label, numbers.Integral) or not 0 <= null_label < n_classes:
        raise ValueError(f"label_information: null_label must be an integer in [0, {n_classes})")
    nll = torch.zeros(2, dtype=torch.float64, device=device)
    count = torch.zeros((), dtype=torch.int64, device=device)
    n = 0
    for x, y, c, g, input_lengths in test_loader:
        c = c.to(device).unsqueeze(1)
        codes, lengths = codes_from_mels(vqvae, c, input_lengths)
        label = prior_labels(prior, g, len(c))
        cond_nll, clip_count = prior.nll(codes, label, lengths)
        null_nll, _ = prior.nll(codes, torch.full_like(label, int(null_label)), lengths)
        nll[0] += cond_nll.double().sum()
        nll[1] += null_nll.double().sum()
        count += clip_count.sum()
        n += 1
    if n == 0:
        raise ValueError("label_information: empty loader")
    if int(count) == 0:
        raise ValueError("label_information: no clip of the loader is long enough for one latent column")
    cond, uncond = float(nll[0] / count), float(nll[1] / count)
    print('====> Prior label information: {:.4f} nats per code conditional, {:.4f} under the null label, gain {:.4f}'.format(
        cond, uncond, uncond - cond))
    return {"nats_conditional": cond, "nats_unconditional": uncond, "gain": uncond - cond}


def convert_voice(vqvae, mel: torch.Tensor, g_target: torch.Tensor, f0_bins: torch.Tensor | None = None):
    """Re-voice clips as other speakers: mel (B, 1, 80, T) (or (B, 80, T)) on the GPU, T a multiple of 4, is encoded to its
    codes and decoded under the speaker ids g_target (B,) int64 -> (codes (B, 20, T // 4) int64, mels (B, 1, 80, T)).  The
    VQ-VAE runs in eval mode (its mode is restored) and is not changed.  ValueError: a model without a speaker embedding, or a
    g_target that is not (B,) int64 within [0, n_speakers) -- checked on the host before anything is launched.
    f0_bins (B, T // 4) int64 in [0, n_f0_bins]: the pitch contour the decoder of an F0-conditioned model (VQVAE(n_f0_bins=)) is
    to follow -- for conversion the source's contour moved to the target speaker's statistics (audio.f0_affine, audio.f0_bins).
    Such a model requires it, a model without an F0 table refuses it: ValueError either way, as for a wrong shape, dtype or range."""
    if getattr(vqvae, "n_speakers", None) is None:
        raise ValueError("convert_voice: the model has no speaker embedding (VQVAE(..., n_speakers=N))")
    has_f0 = getattr(vqvae, "n_f0_bins", None) is not None
    if has_f0 and f0_bins is None:
        raise ValueError("convert_voice: the model's decoder is F0-conditioned (n_f0_bins): give f0_bins (audio.f0_bins)")
    if not has_f0 and f0_bins is not None:
        raise ValueError("convert_voice: f0_bins given to a model without an F0 table (VQVAE(..., n_f0_bins=N))")
    if mel.dim() == 3:
        mel = mel.unsqueeze(1)
    if mel.dim() != 4 or mel.shape[1] != 1:
        raise ValueError("convert_voice: mel must be (B, 1, 80, T) or (B, 80, T)")
    B = mel.shape[0]
    if not isinstance(g_target, torch.Tensor) or tuple(g_target.shape) != (B,) or g_target.dtype != torch.int64:
        raise ValueError(f"convert_voice: g_target must be an int64 tensor of shape ({B},)")
    if B and (int(g_target.min()) < 0 or int(g_target.max()) >= vqvae.n_speakers):
        raise ValueError(f"convert_voice: g_target must lie in [0, {vqvae.n_speakers}), got {int(g_target.min())} .. {int(g_target.max())}")
    if f0_bins is not None:
        vqvae.check_f0_bins(f0_bins, B, mel.shape[3] // 4, "convert_voice")
    was_training = vqvae.training
    vqvae.eval()
    try:
        with torch.no_grad():
            codes = vqvae.encode(mel).contiguous()
            g_dev = g_target.to(mel.device)
            mels = vqvae.decode(codes, g_dev) if f0_bins is None else vqvae.decode(codes, g_dev, f0_bins.to(mel.device))
    finally:
        vqvae.train(was_training)
    return codes, mels


def test_conversion(args, vqvae, pair_loader, device, epoch):
    """The conversion figure of a speaker-conditioned VQ-VAE over parallel utterances: `pair_loader` yields
    (c_src (B, 80, Ts), frames_src (B,), c_tgt (B, 80, Tt), frames_tgt (B,), g_tgt (B,) int64) -- the same sentences by a source
    and a target speaker, zero-padded mels with their valid frame counts (host integers), and the target speakers' ids.  Each
    source batch is converted to its target speakers (convert_voice; Ts is cut to a multiple of 4, and the converted mel keeps
    the source's valid frames, floored to a multiple of 4) and compared with the target by audio.mel_cepstral_distortion;
    MCD(source, target) is measured beside it for context.  Returns (mcd_converted, mcd_source): means over the clips of the
    loader (not over its batches), in dB, read back with one host synchronisation at the end."""
    from . import audio
    total = torch.zeros(2, dtype=torch.float64, device=device)
    n = 0
    for c_src, frames_src, c_tgt, frames_tgt, g_tgt in pair_loader:
        c_src, c_tgt = c_src.to(device), c_tgt.to(device).contiguous()
        fs = np.asarray(frames_src.cpu() if torch.is_tensor(frames_src) else frames_src).astype(np.int64)
        ft = np.asarray(frames_tgt.cpu() if torch.is_tensor(frames_tgt) else frames_tgt).astype(np.int64)
        Ts = c_src.shape[2] // 4 * 4
        fc = np.minimum(fs, Ts) // 4 * 4
        if Ts < 4 or fc.min() < 4:
            raise ValueError("test_conversion: every source clip needs at least 4 valid frames (one latent column)")
        c_cut = c_src[:, :, :Ts].contiguous()
        _, converted = convert_voice(vqvae, c_cut, g_tgt)
        mcd_c, _ = audio.mel_cepstral_distortion(converted, c_tgt, fc, ft)
        mcd_s, _ = audio.mel_cepstral_distortion(c_src.contiguous(), c_tgt, fs, ft)
        total += torch.stack((mcd_c.double().sum(), mcd_s.double().sum()))
        n += len(c_src)
    if n == 0:
        raise ValueError("test_conversion: empty loader")
    mcd_c, mcd_s = (total / n).tolist()
    print('====> Conversion test set: MCD {:.4f} dB converted, {:.4f} dB source against target ({} clips)'.format(mcd_c, mcd_s, n))
    return mcd_c, mcd_s


def _f0_tracker(fn, tracker, tracker_options):
    """audio.f0 or audio.f0_track with its costs, as test_conversion_f0, speaker_f0_stats, test_conditioned, train.train_conditioned
    and data.ResidentMelCorpus.track_f0 name them."""
    from . import audio
    if tracker not in ("yin", "viterbi"):
        raise ValueError(f"{fn}: tracker must be 'yin' or 'viterbi', got {tracker!r}")
    options = dict(tracker_options or {})
    if set(options) - (set(audio.F0_TRACK_COSTS) if tracker == "viterbi" else set()):
        raise ValueError(f"{fn}: tracker_options {sorted(options)} do not go with tracker {tracker!r} "
                         f"(viterbi takes {sorted(audio.F0_TRACK_COSTS)})")
    return audio.f0 if tracker == "yin" else functools.partial(audio.f0_track, **options)


def batch_conditioning(fn, model, batch, device, track):
    """One loader batch as a conditioned model takes it -> (c (B, 1, 80, T) on the device, g on the device or None, f0_bins or
    None).  batch: (x, y, c, g, input_lengths[, f0_bins]).  g is passed only to a model with a speaker table; bins only to one
    with an F0 table: the batch's sixth element if it has one (moved to the device), else tracked by `track` (_f0_tracker's) from
    the audio x (B, 1, T * 256) -- lengths = input_lengths, F0 frame t is mel frame t, the first 4 * (T // 4) frames binned by
    audio.f0_bins over the model's n_f0_bins and f0_range with input_lengths // 256 frames valid.  ValueError (named `fn`): a
    model with an F0 table and neither; tracking a batch of fewer than 4 frames.  train.train_conditioned and test_conditioned
    share it."""
    from . import audio
    x, c, g, input_lengths = batch[0], batch[2], batch[3], batch[4]
    given = batch[5] if len(batch) > 5 else None
    has_f0 = getattr(model, "n_f0_bins", None) is not None
    if has_f0 and given is None and x is None:
        raise ValueError(f"{fn}: the model's decoder is F0-conditioned and the loader yields no audio to track F0 from: "
                         "get_data_loaders(with_audio=True), or bins from a resident track: get_resident_loaders(f0=...)")
    c = c.to(device).unsqueeze(1)
    g_d = g.to(device) if g is not None and getattr(model, "n_speakers", None) is not None else None
    bins = None
    if has_f0 and given is not None:
        bins = given.to(device)
    elif has_f0:
        hop, T = 256, c.shape[3]
        if T < 4:
            raise ValueError(f"{fn}: a batch of fewer than 4 frames has no latent column")
        lens = np.asarray(input_lengths.cpu() if torch.is_tensor(input_lengths) else input_lengths).astype(np.int64)
        f0, _ = track(x.view(x.shape[0], -1).to(device).contiguous(), hop_size=hop, lengths=lens)
        bins = audio.f0_bins(f0[:, :T // 4 * 4].contiguous(), frames=(lens // hop).clip(0, T // 4 * 4), n_bins=model.n_f0_bins,
                             fmin=model.f0_range[0], fmax=model.f0_range[1])
    return c, g_d, bins


def test_conditioned(args, model, test_loader, device, epoch, tracker="yin", tracker_options=None):
    """test_vqvae for a speaker- and / or F0-conditioned VQ-VAE: the same two figures with the model called under each batch's
    own conditioning, model(c, g, f0_bins) in eval mode (test_vqvae calls model(c): no speaker row, no F0 row).  `test_loader`
    yields train.train_conditioned's batches: g goes only to a model with a speaker table; the bins of a model with an F0 table
    are the batch's sixth element (data.ResidentMelLoader(f0=)) or are tracked from its audio x exactly as train_conditioned
    tracks them (tracker, tracker_options); ValueError for such a model and a batch with neither.  Pools as test_vqvae does (the
    mean over the batches of mse(padded reconstruction, c) and of mse(z_q, z_e)) and returns (loss_recons, loss_vq) as floats.
    The model's mode is restored."""
    track = _f0_tracker("test_conditioned", tracker, tracker_options)
    was_training = model.training
    model.eval()
    loss_recons = torch.zeros((), device=device)
    loss_vq = torch.zeros((), device=device)
    n = 0
    try:
        with torch.no_grad():
            for batch in test_loader:
                c, g_d, bins = batch_conditioning("test_conditioned", model, batch, device, track)
                x_tilde, z_e_x, z_q_x = model(c, g_d, bins)
                target = F.pad(x_tilde, (0, c.size(3) - x_tilde.size(3))) if x_tilde.size(3) != c.size(3) else x_tilde
                loss_recons += F.mse_loss(target, c)
                loss_vq += F.mse_loss(z_q_x, z_e_x)
                n += 1
    finally:
        model.train(was_training)
    if n == 0:
        raise ValueError("test_conditioned: empty loader")
    loss_recons, loss_vq = float(loss_recons / n), float(loss_vq / n)
    print('====> Test set loss: {:.4f}'.format(loss_recons + loss_vq))
    return loss_recons, loss_vq


def speaker_f0_stats(wav_loader, n_speakers, device, tracker="yin", tracker_options=None):
    """Every speaker's log-F0 statistics, the target side of pitch-transforming conversion: `wav_loader` yields (wav (B, L) float32
    zero-padded at 22 050 Hz, lengths (B,) host integers, g (B,) int64 speaker ids).  Per batch the F0 track (tracker,
    tracker_options: test_conversion_f0's) and audio.logf0_sums of its 1 + length // 256 frames, added to the speaker's row on the
    device.  Returns (stats (n_speakers, 2) fp64: mean and standard deviation (of the population: / n) of log2 F0 over all voiced
    frames of the speaker, NaN for a speaker without one; counts (n_speakers,) int64 voiced frames) on the host, read back once."""
    from . import audio
    track = _f0_tracker("speaker_f0_stats", tracker, tracker_options)
    if isinstance(n_speakers, bool) or not isinstance(n_speakers, numbers.Integral) or n_speakers < 1:
        raise ValueError(f"speaker_f0_stats: n_speakers must be a positive integer, got {n_speakers!r}")
    hop = 256
    total = torch.zeros(n_speakers, 3, dtype=torch.float64, device=device)
    seen = False
    for wav, lengths, g in wav_loader:
        ls = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64)
        g = torch.as_tensor(g, dtype=torch.int64)
        if tuple(g.shape) != (len(wav),) or (len(wav) and (int(g.min()) < 0 or int(g.max()) >= n_speakers)):
            raise ValueError(f"speaker_f0_stats: g must hold {len(wav)} speaker ids in [0, {n_speakers})")
        f0, _ = track(wav.to(device).contiguous(), hop_size=hop, lengths=ls)
        total.index_add_(0, g.to(device), audio.logf0_sums(f0, 1 + ls // hop))
        seen = True
    if not seen:
        raise ValueError("speaker_f0_stats: empty loader")
    n, s1, s2 = total.cpu().unbind(1)                                       # the one read-back
    mean = s1 / n                                                           # (0 / 0: NaN for a speaker without a voiced frame)
    std = torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
    return torch.stack((mean, std), dim=1), n.to(torch.int64)


def test_conversion_f0(args, vqvae, pair_loader, device, epoch, iters=None, angles0=None, *, tracker="yin", tracker_options=None, momentum=0.0, init="random",
                       f0_stats=None, psola_baseline=False):
    """The pitch figures of a speaker-conditioned VQ-VAE over parallel utterances, from waveforms: `pair_loader` yields
    (wav_src (B, Ls), len_src (B,), wav_tgt (B, Lt), len_tgt (B,), g_tgt (B,) int64) -- the same sentences by a source and a target
    speaker as zero-padded float32 waveforms at 22 050 Hz with their lengths in samples (host integers), and the target speakers'
    ids.  Per batch: audio.melspectrogram of both (frame t centred on sample 256 t); the source mel cut to a multiple of 4 frames
    and converted (convert_voice; the converted mel keeps the source's valid frames floored to a multiple of 4);
    audio.inv_mel_spectrogram of the converted mel (iters Griffin-Lim iterations, default audio.GRIFFIN_LIM_ITERS; angles0: the
    initial phases (B, frames, 513) for every batch, or a sequence of them, one per batch; None draws them); audio.f0 of the
    converted, the target and the source waveforms (F0 frame t is mel frame t); mel cepstra and ops.dtw with the path of converted
    against target and of source against target; ops.f0_path_stats along each path.  Returns
        {"converted": figures, "source": figures, "clips": n},   figures = {"f0_rmse_cents", "vuv_error", "f0_corr", "mcd", "stats"}
    and, in "converted" alone, "spectral_convergence": the mean over clips of audio.spectral_convergence of Griffin-Lim's waveform
    (before the inverse pre-emphasis) against the magnitudes it was inverted from, i.e. how far the inversion behind the converted
    figures still is from the spectrum asked for; momentum is audio.griffin_lim's (0, the default, is the reference's iteration) and
    init audio.inv_mel_spectrogram's ("random", the default, or "spsi": Griffin-Lim starts from audio.spsi_phases, without angles0);
    each set pooled over all clips of the loader from the summed stats (audio.f0_figures of the sum, not a mean of per-clip
    ratios), "mcd" the mean over clips of the mel-cepstral distortion along the same paths in dB, "stats" the ten sums.  One host
    synchronisation, at the end.  ValueError, before anything of the batch is launched: a model without a speaker embedding, a
    clip tensor of more than ops.DTW_MAX_FRAMES frames, a source clip of fewer than 4 frames; before anything at all: an empty loader.
    tracker: "yin" (audio.f0, each frame on its own) or "viterbi" (audio.f0_track for all three waveforms: a path over each
    frame's candidates, which repairs the octave-up picks and dropouts that a per-frame rule makes on a Griffin-Lim waveform and
    that otherwise dominate the figures); tracker_options: audio.f0_track's costs (octave_cost, jump_cost, vuv_cost,
    unvoiced_cost) for "viterbi".  Another tracker, options that do not go with it, a momentum outside [0, 1], or an init that is
    neither or that comes with angles0 is a ValueError before anything is launched.
    A model with an F0 table (VQVAE(n_f0_bins=)): the source's F0 is tracked before the conversion and its first Tc frames become
    the bins the decoder follows (audio.f0_bins over the model's n_f0_bins and f0_range).  f0_stats (n_speakers, 2): every
    speaker's mean and standard deviation of log2 F0 (speaker_f0_stats) -- the contour is first moved to the target speaker's
    statistics, each source clip's own moments (audio.logf0_sums) being the source side (audio.f0_affine); f0_stats=None keeps the
    source's contour (the identity move).  ValueError before anything is launched: f0_stats for a model without the table or of
    another shape; before anything of the batch: a target speaker of the batch whose statistics are not finite.
    psola_baseline=True adds a third set, "psola_source", with the same five figures: the source waveform moved by signal
    processing alone -- audio.pitch_shift_psola to the contour the decoder would be given (the source's track under audio.f0_affine
    of the target speaker's f0_stats, over all of its frames; without f0_stats the source's own) -- then audio.melspectrogram and
    the tracker, scored against the target exactly as "source" is.  It is the row a conversion has to beat on pitch without the
    help of a model.  With the flag off nothing of it runs and the dict is what it was."""
    from . import audio
    momentum = audio._momentum("test_conversion_f0", momentum)
    audio._init("test_conversion_f0", init, angles0)
    track = _f0_tracker("test_conversion_f0", tracker, tracker_options)
    if getattr(vqvae, "n_speakers", None) is None:
        raise ValueError("test_conversion_f0: the model has no speaker embedding (VQVAE(..., n_speakers=N))")
    has_f0 = getattr(vqvae, "n_f0_bins", None) is not None
    if f0_stats is not None:
        if not has_f0:
            raise ValueError("test_conversion_f0: f0_stats given to a model without an F0 table (VQVAE(..., n_f0_bins=N))")
        f0_stats = np.asarray(f0_stats.cpu() if torch.is_tensor(f0_stats) else f0_stats, dtype=np.float64)
        if f0_stats.shape != (vqvae.n_speakers, 2):
            raise ValueError(f"test_conversion_f0: f0_stats must be ({vqvae.n_speakers}, 2): mean and std of log2 F0 per speaker")
    hop, fft = 256, 1024
    iters = audio.GRIFFIN_LIM_ITERS if iters is None else int(iters)
    total = torch.zeros(3 if psola_baseline else 2, 12, dtype=torch.float64, device=device)          # per set: the ten sums, the sums of the clips' MCD and convergence
    n = 0
    for k, (wav_src, len_src, wav_tgt, len_tgt, g_tgt) in enumerate(pair_loader):
        ls = np.asarray(len_src.cpu() if torch.is_tensor(len_src) else len_src).astype(np.int64)
        lt = np.asarray(len_tgt.cpu() if torch.is_tensor(len_tgt) else len_tgt).astype(np.int64)
        Ts, Tt = 1 + wav_src.shape[1] // hop, 1 + wav_tgt.shape[1] // hop
        if max(Ts, Tt) > ops.DTW_MAX_FRAMES:
            raise ValueError(f"test_conversion_f0: clips of {Ts} / {Tt} frames; the warping serves at most {ops.DTW_MAX_FRAMES}")
        fs, ft = 1 + ls // hop, 1 + lt // hop
        Tc = Ts // 4 * 4
        fc = np.minimum(fs, Tc) // 4 * 4
        if Tc < 4 or fc.min() < 4:
            raise ValueError("test_conversion_f0: every source clip needs at least 4 valid frames (one latent column)")
        if f0_stats is not None:
            gt = np.asarray(g_tgt.cpu() if torch.is_tensor(g_tgt) else g_tgt).astype(np.int64)
            if gt.shape != (len(wav_src),) or gt.min() < 0 or gt.max() >= vqvae.n_speakers:
                raise ValueError(f"test_conversion_f0: g_tgt must hold {len(wav_src)} speaker ids in [0, {vqvae.n_speakers})")
            target = f0_stats[gt]                                           # (B, 2)
            if not np.isfinite(target).all():
                raise ValueError(f"test_conversion_f0: f0_stats of the target speakers {sorted(set(gt[~np.isfinite(target).all(1)].tolist()))} "
                                 "are not finite (a speaker without a voiced frame in speaker_f0_stats)")
        wav_src, wav_tgt = wav_src.to(device).contiguous(), wav_tgt.to(device).contiguous()
        mel_s = audio.melspectrogram(wav_src, fft_size=fft, hop_size=hop, lengths=ls)
        mel_t = audio.melspectrogram(wav_tgt, fft_size=fft, hop_size=hop, lengths=lt)
        f0_s, _ = track(wav_src, hop_size=hop, lengths=ls)
        bins = None
        if has_f0:      # the source's contour over the frames that are converted, moved to the target speaker's statistics
            f0_c_in = f0_s[:, :Tc].contiguous()
            affine = None
            if f0_stats is not None:
                tgt = torch.from_numpy(target).to(device)
                affine = audio.f0_affine(audio.logf0_sums(f0_c_in, fc), tgt[:, 0], tgt[:, 1])
            bins = audio.f0_bins(f0_c_in, frames=fc, n_bins=vqvae.n_f0_bins, fmin=vqvae.f0_range[0], fmax=vqvae.f0_range[1], affine=affine)
        sets = []
        if psola_baseline:
            f0_goal = f0_s
            if f0_stats is not None:
                tgt = torch.from_numpy(target).to(device)
                aff = audio.f0_affine(audio.logf0_sums(f0_s, fs), tgt[:, 0], tgt[:, 1])
                moved = torch.exp2(aff[:, 2:3] + (torch.log2(f0_s.clamp_min(1e-30)) - aff[:, 0:1]) * aff[:, 1:2])
                f0_goal = torch.where(f0_s > 0, moved, torch.zeros_like(f0_s)).contiguous()
            wav_p = audio.pitch_shift_psola(wav_src, f0_s, target_f0=f0_goal, hop_size=hop, lengths=ls)
            sets.append((audio.melspectrogram(wav_p, fft_size=fft, hop_size=hop, lengths=ls), fs, track(wav_p, hop_size=hop, lengths=ls)[0]))
        _, converted = convert_voice(vqvae, mel_s[:, :, :Tc].contiguous(), g_tgt, *(() if bins is None else (bins,)))
        a0 = angles0[k] if isinstance(angles0, (list, tuple)) else angles0
        S_c, y_c, wav_c = audio._invert_mel(converted.squeeze(1), 22050, fft, hop, 80, iters, a0, momentum, init)      # inv_mel_spectrogram's steps
        total[0, 11] += audio.spectral_convergence(y_c, S_c, fft, hop).sum()
        f0_c, _ = track(wav_c, hop_size=hop, lengths=hop * (fc - 1))   # hop (Tc - 1) samples: Tc frames, fc of them the clip's
        f0_t, _ = track(wav_tgt, hop_size=hop, lengths=lt)
        cep_t = audio.mel_cepstra(mel_t, ft)
        for row, (mel, frames, f0_x) in enumerate([(converted, fc, f0_c), (mel_s, fs, f0_s)] + sets):
            cost, steps, path = ops.dtw(audio.mel_cepstra(mel, frames), cep_t, frames, ft, want_path=True)
            stats = ops.f0_path_stats(f0_x, f0_t, path, steps)
            mcd = (cost / steps.to(torch.float32)) * audio.MCD_DB
            total[row, :10] += stats.sum(0)
            total[row, 10] += mcd.double().sum()
        n += len(wav_src)
    if n == 0:
        raise ValueError("test_conversion_f0: empty loader")
    sums = torch.cat((total, torch.stack(audio.f0_figures(total[:, :10]), dim=1)), dim=1).tolist()      # the one read-back
    out = {"clips": n}
    for row, name in enumerate(("converted", "source") + (("psola_source",) if psola_baseline else ())):
        rmse, vuv, corr = sums[row][12:]
        out[name] = {"f0_rmse_cents": rmse, "vuv_error": vuv, "f0_corr": corr, "mcd": sums[row][10] / n, "stats": sums[row][:10]}
    out["converted"]["spectral_convergence"] = sums[0][11] / n
    print('====> Conversion test set: F0 RMSE {:.2f} cents, V/UV error {:.4f}, log-F0 correlation {:.4f}, MCD {:.4f} dB converted; '
          '{:.2f} cents, {:.4f}, {:.4f}, {:.4f} dB source against target ({} clips)'.format(
              *(out["converted"][k] for k in ("f0_rmse_cents", "vuv_error", "f0_corr", "mcd")),
              *(out["source"][k] for k in ("f0_rmse_cents", "vuv_error", "f0_corr", "mcd")), n))
    if psola_baseline:
        print('====> Conversion test set: {:.2f} cents, {:.4f}, {:.4f}, {:.4f} dB source moved by PSOLA against target'.format(
            *(out["psola_source"][k] for k in ("f0_rmse_cents", "vuv_error", "f0_corr", "mcd"))))
    print('====> Conversion test set: spectral convergence of the inversion {:.4f} ({} Griffin-Lim iterations, momentum {:g}, init {})'.format(
        out["converted"]["spectral_convergence"], iters, momentum, init))
    return out


def test_reconstruction_audio(args, vqvae, wav_loader, device, epoch, iters=None, angles0=None, *, momentum=0.0, init="random"):
    """The audio figure of a VQ-VAE's reconstructions, against the recordings themselves: `wav_loader` yields (wav (B, L) float32
    zero-padded at 22 050 Hz, lengths (B,) host integers) or (wav, lengths, g (B,) int64 speaker ids).  Per batch:
    audio.melspectrogram(wav, lengths=...) (T = 1 + L // 256 frames); Tc = T // 4 * 4; the model in eval mode (its mode is restored)
    on mel[:, None, :, :Tc], with g if the model has speakers; then two waveforms of 256 (Tc - 1) samples from inv_mel_spectrogram's
    steps -- "analysis_synthesis", from the mel itself: the ceiling the mel inversion sets, whatever the model does -- and
    "reconstruction", from the model's output.  Each is scored against wav[:, :256 (Tc - 1)] with the lengths min(len, 256 (Tc - 1))
    by audio.stoi, both STOI and ESTOI (at 10 kHz, through audio.resample).  iters (default audio.GRIFFIN_LIM_ITERS), angles0 (the
    initial phases (B, Tc, 513) for every batch, or a sequence of them, one per batch; None draws them), momentum and init are
    audio.inv_mel_spectrogram's, and serve both inversions.  Returns
        {"analysis_synthesis": {"stoi", "estoi"}, "reconstruction": {"stoi", "estoi"}, "clips": n, "scored": n_finite}
    each figure the mean over the clips of the loader on which it is finite (a clip that keeps fewer than 30 frames at 10 kHz,
    about 0.4 s of speech, has none: NaN if there is no such clip at all), "scored" the clips on which all four are.  The sums and
    counts stay on the device: one host synchronisation, at the end.  ValueError before anything is launched: a momentum outside
    [0, 1], an init that is neither "random" nor "spsi" or that comes with angles0; an empty loader."""
    from . import audio
    momentum = audio._momentum("test_reconstruction_audio", momentum)
    audio._init("test_reconstruction_audio", init, angles0)
    hop, fft = 256, 1024
    iters = audio.GRIFFIN_LIM_ITERS if iters is None else int(iters)
    total = torch.zeros(2, 5, dtype=torch.float64, device=device)           # per figure: the sum and the count of the finite ones | [0, 4]: clips with all four
    n = 0
    was_training = vqvae.training
    vqvae.eval()
    try:
        for k, batch in enumerate(wav_loader):
            wav, lengths = batch[0], batch[1]
            g = batch[2] if len(batch) > 2 else None
            ls = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64)
            wav = wav.to(device).contiguous()
            Tc = (1 + wav.shape[1] // hop) // 4 * 4
            if Tc < 4:
                raise ValueError("test_reconstruction_audio: the batch needs at least 4 frames (one latent column)")
            mel = audio.melspectrogram(wav, fft_size=fft, hop_size=hop, lengths=ls)[:, :, :Tc].contiguous()
            with torch.no_grad():
                g_d = g.to(device) if g is not None and getattr(vqvae, "n_speakers", None) is not None else None
                out = vqvae(mel.unsqueeze(1), g_d)[0].squeeze(1)
            if out.shape[2] != Tc:
                out = F.pad(out, (0, Tc - out.shape[2])) if out.shape[2] < Tc else out[:, :, :Tc]
            a0 = angles0[k] if isinstance(angles0, (list, tuple)) else angles0
            n_out = hop * (Tc - 1)
            clean = wav[:, :n_out].contiguous()
            lc = np.minimum(ls, n_out)
            figures = []
            for m in (mel, out.contiguous()):
                y = audio._invert_mel(m, 22050, fft, hop, 80, iters, a0, momentum, init)[2]
                figures += [audio.stoi(clean, y, 22050, lc, extended=ext)[0] for ext in (False, True)]
            d = torch.stack(figures)                                        # (4, B): a/s stoi, a/s estoi, reconstruction stoi, estoi
            ok = torch.isfinite(d)
            total[0, :4] += torch.where(ok, d, torch.zeros_like(d)).sum(1)
            total[1, :4] += ok.sum(1)
            total[0, 4] += ok.all(0).sum()
            n += len(wav)
    finally:
        vqvae.train(was_training)
    if n == 0:
        raise ValueError("test_reconstruction_audio: empty loader")
    sums, counts = total.tolist()                                           # the one read-back
    mean = [s / c if c else float("nan") for s, c in zip(sums[:4], counts[:4])]
    res = {"analysis_synthesis": {"stoi": mean[0], "estoi": mean[1]}, "reconstruction": {"stoi": mean[2], "estoi": mean[3]},
           "clips": n, "scored": int(sums[4])}
    print('====> Reconstruction test set: STOI {:.4f}, ESTOI {:.4f} reconstructed; {:.4f}, {:.4f} analysis-synthesis ({} of {} clips scored, '
          '{} Griffin-Lim iterations, momentum {:g}, init {})'.format(mean[2], mean[3], mean[0], mean[1], res["scored"], n, iters, momentum, init))
    return res


@torch.no_grad()
def continue_mels(vqvae, prior, mel: torch.Tensor, label: torch.Tensor, keep_frames: int, frames: int, g=None, generator=None, **controls):
    """Continue mels in time: mel (B, 1, 80, T) is encoded to its codes, the first keep_frames // 4 latent columns are kept
    and the prior samples the grid out to frames // 4 columns (GatedPixelCNN.continue_codes, which says what the sampled codes
    are conditioned on; controls: temperature, top_k, top_p), then the grid is decoded.  Returns codes (B, 20, frames // 4)
    and mels (B, 1, 80, frames).  guidance= and null_label= (classifier-free guidance) pass through to sample as well."""
    if frames < 4:
        raise ValueError("continue_mels: frames must be at least 4 (one latent column)")
    known = vqvae.encode(mel)
    w0 = int(keep_frames) // 4
    if keep_frames < 0 or w0 > known.shape[-1] or w0 > frames // 4:
        raise ValueError(f"continue_mels: keep_frames = {keep_frames} must be within the mel's {4 * known.shape[-1]} frames and frames = {frames}")
    codes = prior.continue_codes(known[:, :, :w0].contiguous(), label, frames // 4, generator=generator, **controls)
    return codes, vqvae.decode(codes, g)


@torch.no_grad()
def continue_audio(vqvae, prior, wav: torch.Tensor, label: torch.Tensor, keep_frames: int, frames: int, g=None, generator=None,
                   sample_rate=22050, fft_size=1024, hop_size=256, angles0=None, iters=None, momentum=0.0, init="random", **controls):
    """Continue recordings in time: wav (B, L) float32 on the GPU -> its mel (audio.melspectrogram, 1 + L // hop_size frames)
    -> continue_mels (the first keep_frames held, the grid sampled out to frames) -> waveform (audio.inv_mel_spectrogram;
    angles0 (B, frames, 1 + fft_size / 2) fixes Griffin-Lim's initial phases; iters, default audio.GRIFFIN_LIM_ITERS, and momentum
    are audio.griffin_lim's, init audio.inv_mel_spectrogram's).  Returns codes (B, 20, frames // 4), mels
    (B, 1, 80, frames) and waveforms (B, hop_size * (frames - 1)).  guidance= and null_label= (classifier-free guidance) pass
    through to GatedPixelCNN.sample with the other controls."""
    from . import audio
    audio._init("continue_audio", init, angles0)
    mel = audio.melspectrogram(wav, sample_rate, fft_size, hop_size, 80)
    codes, out = continue_mels(vqvae, prior, mel.unsqueeze(1), label, keep_frames, frames, g=g, generator=generator, **controls)
    y = audio.inv_mel_spectrogram(out.squeeze(1), sample_rate, fft_size, hop_size, 80, audio.GRIFFIN_LIM_ITERS if iters is None else int(iters),
                                  angles0=angles0, momentum=momentum, init=init)
    return codes, out, y
