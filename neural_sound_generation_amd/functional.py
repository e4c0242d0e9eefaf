"""torch.autograd.Function wrappers around the engine's explicit forward/backward pieces, so the
fused encoder / decoder / ResBlock stacks compose with ordinary autograd code (the reference's
src/train.py calls loss.backward() on the model outputs).

Tensors cross this boundary in the reference's logical NCHW shape; physically they are NHWC
("channels_last"), so the permutes below are views, not copies.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import engine, ops, vae_engine


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """(B,C,H,W) logical -> contiguous [B][H][W][C]; free when x is channels_last or C == 1."""
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw_view(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)


def _check_float_cuda(x, what):
    if not x.is_cuda:
        raise RuntimeError(f"{what}: this path runs only on an AMD GPU (got a {x.device} tensor); there is no CPU fallback")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {x.dtype}")


class _Stack(Function):
    """Shared plumbing: subclasses set fwd / bwd / bundle."""

    @staticmethod
    def _run_forward(ctx, fwd, bundle, x, training, params, dtype):
        _check_float_cuda(x, fwd.__name__)
        ctx.bundle = bundle
        ctx.training = training
        ctx.dtype = dtype
        # The backward reads some parameters again (BatchNorm scales, the 1x1 weights): registering them with autograd makes
        # `ctx.saved_tensors` raise the usual "modified by an inplace operation" error if an optimiser stepped in between,
        # as the reference's per-layer autograd would, instead of silently differentiating against the new values.
        ctx.save_for_backward(*params)
        if fwd is engine.resblock_forward:
            y, saved = fwd(ops.convert(to_nhwc(x.detach()), dtype, relu=True), bundle, training, out_dtype=torch.float32)
        else:
            y, saved = fwd(to_nhwc(x.detach()), bundle, training, dtype=dtype)
        ctx.saved = saved
        return to_nchw_view(y)


class EncoderFn(Function):
    @staticmethod
    def forward(ctx, x, bundle, training, dtype, *params):
        if ctx.needs_input_grad[0]:
            # the reference can differentiate w.r.t. the mel image; this path does not build that gradient (the input layer's
            # conv output is never stored) -- say so instead of returning None
            raise RuntimeError("the encoder input is data: a gradient w.r.t. the mel batch is not implemented (pass c.detach())")
        return _Stack._run_forward(ctx, engine.encoder_forward, bundle, x, training, params, dtype)

    @staticmethod
    def backward(ctx, dz):
        if not ctx.training:
            raise RuntimeError("backward through the encoder in eval() mode is not implemented")
        ctx.saved_tensors                      # version check of the parameters (see _run_forward)
        grads = engine.encoder_backward(to_nhwc(dz), ctx.saved, ctx.bundle)
        return (None, None, None, None) + tuple(engine.encoder_grad_list(grads))


class DecoderFn(Function):
    @staticmethod
    def forward(ctx, z, bundle, training, dtype, *params):
        return _Stack._run_forward(ctx, engine.decoder_forward, bundle, z, training, params, dtype)

    @staticmethod
    def backward(ctx, dxt):
        if not ctx.training:
            raise RuntimeError("backward through the decoder in eval() mode is not implemented")
        ctx.saved_tensors
        dz, grads = engine.decoder_backward(to_nhwc(dxt), ctx.saved, ctx.bundle, need_dz=ctx.needs_input_grad[0])
        if dz is not None:
            dz = to_nchw_view(ops.convert(dz, torch.float32))
        return (dz, None, None, None) + tuple(engine.decoder_grad_list(grads))


class ResBlockFn(Function):
    @staticmethod
    def forward(ctx, x, bundle, training, dtype, *params):
        return _Stack._run_forward(ctx, engine.resblock_forward, bundle, x, training, params, dtype)

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("backward through a ResBlock in eval() mode is not implemented")
        ctx.saved_tensors
        dx, grads = engine.resblock_backward(ops.convert(to_nhwc(dy), ctx.dtype), ctx.saved, ctx.bundle, need_dx=ctx.needs_input_grad[0])
        if dx is not None:
            dx = to_nchw_view(ops.convert(dx, torch.float32))
        return (dx, None, None, None) + tuple(engine.resblock_grad_list(grads))


def encoder_apply(x, bundle, training, dtype=torch.float32):
    return EncoderFn.apply(x, bundle, training, dtype, *engine.encoder_param_list(bundle))


def decoder_apply(z, bundle, training, dtype=torch.float32):
    return DecoderFn.apply(z, bundle, training, dtype, *engine.decoder_param_list(bundle))


def resblock_apply(x, bundle, training, dtype=torch.float32):
    return ResBlockFn.apply(x, bundle, training, dtype, *engine.resblock_param_list(bundle))


# ------------------------------------------------------------------------------------------------
# the continuous VAE (vae_engine.py): encoder up to encoder.9 | encoder.10 + the Gaussian latent | decoder
# ------------------------------------------------------------------------------------------------
class VAEEncoderFn(Function):
    """x (B, 1, 80, T) -> (h, mean, invstd): encoder.9's output NHWC = the INPUT of encoder.10, and that BatchNorm's statistics
    (not differentiable here: VAELatentFn's backward is the whole BatchNorm backward, statistics included)."""

    @staticmethod
    def forward(ctx, x, bundle, training, *params):
        if ctx.needs_input_grad[0]:
            raise RuntimeError("the encoder input is data: a gradient w.r.t. the mel batch is not implemented (pass c.detach())")
        _check_float_cuda(x, "vae_encoder_forward")
        ctx.bundle, ctx.training = bundle, training
        ctx.save_for_backward(*params)
        h, mean, invstd, ctx.saved = vae_engine.encoder_forward(to_nhwc(x.detach()), bundle, training)
        ctx.mark_non_differentiable(mean, invstd)
        return h, mean, invstd

    @staticmethod
    def backward(ctx, dh, _dmean, _dinvstd):
        if not ctx.training:
            raise RuntimeError("backward through the VAE encoder in eval() mode is not implemented")
        ctx.saved_tensors
        # encoder.10's own gradients belong to VAELatentFn (they are its inputs): none from here
        grads = vae_engine.encoder_backward(dh.contiguous(), ctx.saved, ctx.bundle, engine.LayerGrads(None, None))
        return (None, None, None) + tuple(vae_engine.encoder_grad_list(grads))


class VAELatentFn(Function):
    """(h, mean, invstd, gamma, beta, eps NHWC) -> (z NHWC, kl 0-d): encoder.10, chunk, KL and the reparameterised sample."""

    @staticmethod
    def forward(ctx, h, mean, invstd, gamma, beta, eps, training):
        ctx.training = training
        z, kl = ops.vae_latent_forward(h, mean, invstd, gamma, beta, eps)
        ctx.save_for_backward(h, mean, invstd, gamma, beta, eps)
        return z, kl.view(())

    @staticmethod
    def backward(ctx, dz, dkl):
        if not ctx.training:
            raise RuntimeError("backward through the VAE latent in eval() mode is not implemented")
        h, mean, invstd, gamma, beta, eps = ctx.saved_tensors
        dz = torch.zeros_like(eps) if dz is None else dz.contiguous()
        kl_grad = None if dkl is None else dkl.reshape(1).contiguous()      # stays on the device: the kernel reads it
        dy, dgamma, dbeta = ops.vae_latent_backward(h, mean, invstd, gamma, beta, eps, dz, kl_scale=0.0 if dkl is None else 1.0,
                                                    kl_grad=kl_grad)
        dh = ops.bn_backward_apply(h, dy, mean, invstd, gamma, dgamma, dbeta)
        return dh, None, None, dgamma, dbeta, None, None


class VAEDecoderFn(Function):
    @staticmethod
    def forward(ctx, z, bundle, training, *params):
        _check_float_cuda(z, "vae_decoder_forward")
        ctx.bundle, ctx.training = bundle, training
        ctx.save_for_backward(*params)
        xt, ctx.saved = vae_engine.decoder_forward(to_nhwc(z.detach()), bundle, training)
        return to_nchw_view(xt)

    @staticmethod
    def backward(ctx, dxt):
        if not ctx.training:
            raise RuntimeError("backward through the VAE decoder in eval() mode is not implemented")
        ctx.saved_tensors
        dz, grads = vae_engine.decoder_backward(to_nhwc(dxt), ctx.saved, ctx.bundle, need_dz=ctx.needs_input_grad[0])
        return (to_nchw_view(dz) if dz is not None else None, None, None) + tuple(vae_engine.decoder_grad_list(grads))


def vae_encoder_apply(x, bundle, training):
    return VAEEncoderFn.apply(x, bundle, training, *vae_engine.encoder_param_list(bundle))


def vae_latent_apply(h, mean, invstd, bn10, eps_nhwc, training):
    return VAELatentFn.apply(h, mean, invstd, bn10.weight, bn10.bias, eps_nhwc, training)


def vae_decoder_apply(z, bundle, training):
    return VAEDecoderFn.apply(z, bundle, training, *vae_engine.decoder_param_list(bundle))
