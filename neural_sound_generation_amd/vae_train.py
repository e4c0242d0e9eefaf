"""The reference's training step of the continuous VAE (src/train.py:42-83, ljspeech branch; src/loss.py:23-29) on the HIP path.

  * `vae_loss(x_tilde, c, kl_d)` -- loss.mse_loss with the zero-pad of train.py:62-64: the squared error summed over the
    elements, divided by the batch size, plus the KL term.
  * `train_vae(args, model, optimizer, train_loader, device, epoch)` -- drop-in for the reference's function: autograd through
    the model's fused stacks, optimizer.step().  Any torch optimiser works.  Returns the mean batch loss (the reference prints
    a sum of batch losses divided by the dataset size and returns nothing).
  * `VAETrainStep` -- the same arithmetic with no autograd in the loop: explicit forward and backward writing straight into
    FlatAdam's gradient bucket, one weight re-pack launch, one counter launch, one Adam launch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import distributed as nsg_dist
from . import engine, functional as Fn, ops, vae_engine
from .optim import FlatAdam


def vae_loss(x_tilde, c, kl_d):
    """loss.py:23-29 on x_tilde zero-padded on the right to c's width (train.py:62-64)."""
    target = F.pad(x_tilde, (0, c.size(3) - x_tilde.size(3))) if x_tilde.size(3) != c.size(3) else x_tilde
    return F.mse_loss(target, c, reduction='sum') / c.size(0) + kl_d


def train_vae(args, model, optimizer, train_loader, device, epoch):
    """`train_loader` yields (x, y, c, g, input_lengths) with c: (B, 80, T) mel frames."""
    model.train()
    train_loss = 0.0
    n_batches = 0
    for batch_idx, (x, y, c, g, input_lengths) in enumerate(train_loader):
        optimizer.zero_grad()
        c = c.to(device).unsqueeze(1)
        x_tilde, kl_d = model(c)
        loss = vae_loss(x_tilde, c, kl_d)
        loss.backward()
        train_loss += loss.item()
        n_batches += 1
        optimizer.step()
        if batch_idx % args.log_interval == 0:
            print('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}'.format(
                epoch, batch_idx * len(c), len(train_loader.dataset), 100. * batch_idx / len(train_loader), loss.item() / len(c)))
    if n_batches == 0:
        raise ValueError("train_vae: empty loader")
    print('====> Epoch: {} Average loss: {:.4f}'.format(epoch, train_loss / n_batches))
    return train_loss / n_batches


class VAETrainStep:
    """One optimiser step of the VAE without autograd.  kl_weight is a plain attribute read at every step (a caller may anneal
    it; 1.0 is the reference's loss).  The seven conv biases that feed a training-mode BatchNorm get a gradient of exactly 0.0
    and no reduction (vae_engine.DEAD_BIASES).  Single process only; no graph capture."""

    def __init__(self, model, lr: float = 1e-3, kl_weight: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 optimizer: FlatAdam | None = None, process_group=None):
        if nsg_dist.world_size(process_group) > 1:
            raise NotImplementedError("VAETrainStep: data-parallel training of the VAE is not implemented (world_size > 1)")
        self.model = model
        self.kl_weight = kl_weight
        self.opt = optimizer if optimizer is not None else FlatAdam(model.parameters(), lr=lr, betas=betas, eps=eps)
        self.encP = vae_engine.encoder_params(model.encoder)
        self.decP = vae_engine.decoder_params(model.decoder)
        self.g_enc = vae_engine.encoder_grads(self.opt.grads_for(vae_engine.encoder_param_list(self.encP)))
        self.g_dec = vae_engine.decoder_grads(self.opt.grads_for(vae_engine.decoder_param_list(self.decP)))

    @torch.no_grad()
    def forward_backward(self, c: torch.Tensor, eps: torch.Tensor | None = None, generator=None):
        """c (B, 1, 80, T) float32 on the GPU; eps (B, z_dim, 14, T // 4 - 6) or None (drawn on the device).  Fills the gradient
        bucket with the gradient of rec + kl_weight * kl; returns (rec, kl) as device scalars: the reconstruction term
        (sum over elements / B) and the KL term, unweighted.  Nothing here synchronises with the host."""
        model = self.model
        if not model.training:
            raise RuntimeError("VAETrainStep needs model.train()")
        h, w = model.latent_grid(c.shape)
        B, T = c.shape[0], c.shape[3]
        if eps is None:
            eps = model._noise(B, h, w, c.device, generator)
        elif tuple(eps.shape) != (B, model.z_dim, h, w):
            raise ValueError(f"VAETrainStep: eps must be {(B, model.z_dim, h, w)}, got {tuple(eps.shape)}")
        x, eps = Fn.to_nhwc(c), Fn.to_nhwc(eps)
        with engine.deferred_batch_counters():
            enc_packs, dec_packs = vae_engine.pack_all(self.encP, self.decP, B, 80, T)
            h9, m10, i10, es = vae_engine.encoder_forward(x, self.encP, True, packs=enc_packs)
            z, kl = vae_engine.latent_forward(h9, m10, i10, self.encP.bn10, eps)
            xt, ds = vae_engine.decoder_forward(z, self.decP, True, packs=dec_packs)
            # sum of squares / B = the padded mean * (80 T); its gradient is the mean's scaled by 80 T
            rec, dxt = ops.mse_padded(xt, x, B * 80, xt.shape[2], T, grad_scale=float(80 * T))
            rec.mul_(float(80 * T))
            dz, _ = vae_engine.decoder_backward(dxt, ds, self.decP, gout=self.g_dec, exact_zero_bias=True)
            dh9, g10 = vae_engine.latent_backward(dz, h9, m10, i10, self.encP.bn10, eps, kl_scale=float(self.kl_weight),
                                                  gout=self.g_enc.bn10)
            vae_engine.encoder_backward(dh9, es, self.encP, g10, gout=self.g_enc, exact_zero_bias=True)
        return rec[0], kl[0]

    def step(self, c: torch.Tensor, eps: torch.Tensor | None = None, generator=None):
        rec, kl = self.forward_backward(c, eps, generator)
        self.opt.step()
        return rec, kl
