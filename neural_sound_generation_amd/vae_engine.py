"""Explicit forward / backward of the continuous VAE's encoder, Gaussian latent and decoder over NHWC buffers
(reference: src/models.py:64-118), as straight sequences of C-ABI kernel calls; fp32 only.  engine.py's records and walkers
are reused: parameters, gradients and saved state travel as named records, the state_dict order is stated once (*_LAYERS).

Layer map (DESIGN.md "The continuous VAE"):
  encoder.0-2   Conv2d(1, D, 4, 2, 1) + BN + ReLU     the fused input layer (even image extents) or conv + bn_stats + bn_apply
  encoder.3-5   Conv2d(D, D, 4, 2, 1) + BN + ReLU     gather GEMM, bn_stats, bn_apply(relu)
  encoder.6-8   Conv2d(D, D, 5, 1, 0) + BN + ReLU     the same
  encoder.9     Conv2d(D, 2Z, 3, 1, 0)                gather GEMM, bn_stats; encoder.10's output is never stored:
  encoder.10 .. chunk, KL, rsample                    vae_latent_forward / vae_latent_backward + bn_backward_apply
  decoder.0-2   ConvTranspose2d(Z, D, 3, 1, 0) + BN + ReLU      the stride-1 transposed kind (a Conv2d's data gradient), bn_*
  decoder.3-5   ConvTranspose2d(D, D, 5, 1, 0) + BN + ReLU      the same
  decoder.6-8   ConvTranspose2d(D, D, 4, 2, 1) + BN + ReLU      the four-parity-class gather GEMM, bn_*
  decoder.9-10  ConvTranspose2d(D, 1, 4, 2, 1) + Tanh           tap products + col2im with the Tanh in its store
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional

import torch

from . import ops
from .engine import (BNParams, ConvParams, LayerGrads, FUSED_C1_LAYER, _bind, _bump, _conv_bn, _flatten, bn_params, conv_params)
from .ops import NSG_TANH_OUT


@dataclass
class VAEEncoderParams:
    conv0: ConvParams   # encoder.0  Conv2d(1, D, 4, 2, 1)
    bn1: BNParams
    conv3: ConvParams   # encoder.3  Conv2d(D, D, 4, 2, 1)
    bn4: BNParams
    conv6: ConvParams   # encoder.6  Conv2d(D, D, 5, 1, 0)
    bn7: BNParams
    conv9: ConvParams   # encoder.9  Conv2d(D, 2Z, 3, 1, 0)
    bn10: BNParams      # encoder.10: applied by the latent kernels


@dataclass
class VAEDecoderParams:
    convt0: ConvParams  # decoder.0  ConvTranspose2d(Z, D, 3, 1, 0)
    bn1: BNParams
    convt3: ConvParams  # decoder.3  ConvTranspose2d(D, D, 5, 1, 0)
    bn4: BNParams
    convt6: ConvParams  # decoder.6  ConvTranspose2d(D, D, 4, 2, 1)
    bn7: BNParams
    convt9: ConvParams  # decoder.9  ConvTranspose2d(D, 1, 4, 2, 1)


VAE_ENCODER_LAYERS = (("conv0", "0"), ("bn1", "1"), ("conv3", "3"), ("bn4", "4"), ("conv6", "6"), ("bn7", "7"), ("conv9", "9"), ("bn10", "10"))
VAE_DECODER_LAYERS = (("convt0", "0"), ("bn1", "1"), ("convt3", "3"), ("bn4", "4"), ("convt6", "6"), ("bn7", "7"), ("convt9", "9"))
# The conv biases that feed a training-mode BatchNorm: the batch mean takes them out again, so their gradient is zero in exact
# arithmetic (what autograd computes there is round-off).  (stack, layer) pairs.
DEAD_BIASES = (("encoder", "conv0"), ("encoder", "conv3"), ("encoder", "conv6"), ("encoder", "conv9"),
               ("decoder", "convt0"), ("decoder", "convt3"), ("decoder", "convt6"))


def _grads_field():
    return field(default_factory=LayerGrads)


@dataclass
class VAEEncoderGrads:
    conv0: LayerGrads = _grads_field()
    bn1: LayerGrads = _grads_field()
    conv3: LayerGrads = _grads_field()
    bn4: LayerGrads = _grads_field()
    conv6: LayerGrads = _grads_field()
    bn7: LayerGrads = _grads_field()
    conv9: LayerGrads = _grads_field()
    bn10: LayerGrads = _grads_field()


@dataclass
class VAEDecoderGrads:
    convt0: LayerGrads = _grads_field()
    bn1: LayerGrads = _grads_field()
    convt3: LayerGrads = _grads_field()
    bn4: LayerGrads = _grads_field()
    convt6: LayerGrads = _grads_field()
    bn7: LayerGrads = _grads_field()
    convt9: LayerGrads = _grads_field()


def latent_width(T: int) -> int:
    """Columns of the latent grid for a T-frame mel image: two stride-2 convs, then k = 5 and k = 3 without padding."""
    return T // 4 - 6


def _descs(B, H, W, D, Z):
    """Every conv descriptor of the model for a (B, H, W) mel batch, encoder then decoder."""
    e0 = ops.conv_desc(B, H, W, 1, D, 4, 2, 1)
    e3 = ops.conv_desc(B, e0.OH, e0.OW, D, D, 4, 2, 1)
    e6 = ops.conv_desc(B, e3.OH, e3.OW, D, D, 5, 1, 0)
    e9 = ops.conv_desc(B, e6.OH, e6.OW, D, 2 * Z, 3, 1, 0)
    return (e0, e3, e6, e9) + _decoder_descs(B, e9.OH, e9.OW, D, Z)


def _decoder_descs(B, h, w, D, Z):
    t0 = ops.conv_desc(B, h, w, Z, D, 3, 1, 0, transposed=True)
    t3 = ops.conv_desc(B, t0.OH, t0.OW, D, D, 5, 1, 0, transposed=True)
    t6 = ops.conv_desc(B, t3.OH, t3.OW, D, D, 4, 2, 1, transposed=True)
    t9 = ops.conv_desc(B, t6.OH, t6.OW, D, 1, 4, 2, 1, transposed=True)
    return t0, t3, t6, t9


def pack_all(encP: VAEEncoderParams, decP: VAEDecoderParams, B: int, H: int, W: int):
    """Every packed weight image of one training step in ONE launch -> (encoder packs, decoder packs)."""
    D, Z = encP.conv0.weight.shape[0], decP.convt0.weight.shape[0]
    d = _descs(B, H, W, D, Z)
    ws = [encP.conv0, encP.conv3, encP.conv6, encP.conv9, decP.convt0, decP.convt3, decP.convt6, decP.convt9]
    pk = ops.pack_weights_batch([(di, c.weight, True, i > 0) for i, (di, c) in enumerate(zip(d, ws))])
    return dict(zip(("conv0", "conv3", "conv6", "conv9"), pk[:4])), dict(zip(("convt0", "convt3", "convt6", "convt9"), pk[4:]))


# ------------------------------------------------------------------------------------------------
# Encoder up to encoder.9   (src/models.py:67-78)
# ------------------------------------------------------------------------------------------------
class VAEEncoderSaved(NamedTuple):
    """x the image; h0 the input conv's output, or None where the fused input layer never stores it (mom0: the image's tap
    moments); a0, a3, a6 the activated tensors; h3, h6 the conv outputs in front of bn4, bn7; (m, i) the BatchNorms' statistics;
    d the descriptors; wd the weights packed for the data gradient."""
    x: torch.Tensor
    h0: Optional[torch.Tensor]
    mom0: Optional[torch.Tensor]
    a0: torch.Tensor
    m1: torch.Tensor
    i1: torch.Tensor
    h3: torch.Tensor
    a3: torch.Tensor
    m4: torch.Tensor
    i4: torch.Tensor
    h6: torch.Tensor
    a6: torch.Tensor
    m7: torch.Tensor
    i7: torch.Tensor
    d: tuple
    wd: tuple


def _pack(packs, name, d, conv, want_dgrad=True):
    return packs[name] if packs is not None else ops.pack_weights(d, conv.weight, want_dgrad=want_dgrad)


def encoder_forward(x, P: VAEEncoderParams, training: bool, packs=None):
    """x fp32 NHWC (B, 80, T, 1) -> (h9 NHWC (B, 14, T/4 - 6, 2Z), the INPUT of encoder.10; its mean; its invstd; saved)."""
    B, H, W, _ = x.shape
    D, Z2 = P.conv0.weight.shape[0], P.conv9.weight.shape[0]
    d0, d3, d6, d9 = _descs(B, H, W, D, Z2 // 2)[:4]
    wf0, _ = _pack(packs, "conv0", d0, P.conv0, want_dgrad=False)
    mom0 = None
    if FUSED_C1_LAYER and H % 2 == 0 and W % 2 == 0:
        h0 = None
        if training:
            mom0 = torch.empty(ops.C1_MOMENTS, dtype=torch.float64, device=x.device)
            a0, m1, i1 = ops.c1conv_bn_relu_forward(x, P.conv0.weight, P.conv0.bias, P.bn1.weight, P.bn1.bias, P.bn1.running_mean,
                                                    P.bn1.running_var, training=True, moments=mom0)
            _bump(P.bn1)
        else:
            m1, i1 = ops.bn_eval_stats(P.bn1.running_mean, P.bn1.running_var)
            a0, _, _ = ops.c1conv_bn_relu_forward(x, P.conv0.weight, P.conv0.bias, P.bn1.weight, P.bn1.bias, training=False, mean=m1, invstd=i1)
    else:       # an odd image extent (the fused layer needs even ones): the separate operators
        h0, m1, i1 = _conv_bn(d0, x, wf0, P.conv0, P.bn1, training)
        a0 = ops.bn_apply(h0, m1, i1, P.bn1.weight, P.bn1.bias, relu=True)
    wf3, wd3 = _pack(packs, "conv3", d3, P.conv3)
    h3, m4, i4 = _conv_bn(d3, a0, wf3, P.conv3, P.bn4, training)
    a3 = ops.bn_apply(h3, m4, i4, P.bn4.weight, P.bn4.bias, relu=True)
    wf6, wd6 = _pack(packs, "conv6", d6, P.conv6)
    h6, m7, i7 = _conv_bn(d6, a3, wf6, P.conv6, P.bn7, training)
    a6 = ops.bn_apply(h6, m7, i7, P.bn7.weight, P.bn7.bias, relu=True)
    wf9, wd9 = _pack(packs, "conv9", d9, P.conv9)
    h9, m10, i10 = _conv_bn(d9, a6, wf9, P.conv9, P.bn10, training)
    return h9, m10, i10, VAEEncoderSaved(x, h0, mom0, a0, m1, i1, h3, a3, m4, i4, h6, a6, m7, i7, (d0, d3, d6, d9), (wd3, wd6, wd9))


def _dead_bias(slot, C, device, exact_zero):
    """The bias-gradient tensor of a conv that feeds a training-mode BatchNorm, and whether a kernel is to fill it (the autograd
    path: the reference's round-off) or it holds an exact 0.0 (the fused step: no reduction runs)."""
    t = slot if slot is not None else torch.empty(C, dtype=torch.float32, device=device)
    if exact_zero:
        t.zero_()
    return t, (None if exact_zero else t)


def _bn_relu_conv_backward(d, wd, a_in, h, da, m, i, bn: BNParams, o_conv: LayerGrads, o_bn: LayerGrads, w_shape, exact_zero, need_dx=True):
    """Backward of conv -> BatchNorm -> ReLU given da, the gradient at the ReLU's output: the BatchNorm (mask re-derived from h),
    then the conv's weight and data gradients.  -> (dx or None, the conv's LayerGrads, the BatchNorm's LayerGrads)."""
    db, colsum = _dead_bias(o_conv.bias, h.shape[-1], h.device, exact_zero)
    dh, dg, dbe = ops.bn_backward(h, None, da, m, i, bn.weight, dgamma=o_bn.weight, dbeta=o_bn.bias, dx_colsum=colsum, relu_beta=bn.bias)
    dw, _ = ops.conv_wgrad(d, a_in, dh, w_shape, dw=o_conv.weight, want_bias=False)
    dx = ops.conv_dgrad(d, dh, wd) if need_dx else None
    return dx, LayerGrads(dw, db), LayerGrads(dg, dbe)


def encoder_backward(dh9, saved: VAEEncoderSaved, P: VAEEncoderParams, bn10: LayerGrads, gout: Optional[VAEEncoderGrads] = None,
                     exact_zero_bias: bool = False) -> VAEEncoderGrads:
    """dh9: the gradient at encoder.9's output (latent_backward); bn10: encoder.10's gradients, formed there."""
    s = saved
    o = gout if gout is not None else VAEEncoderGrads()
    d0, d3, d6, d9 = s.d
    wd3, wd6, wd9 = s.wd
    db9, want9 = _dead_bias(o.conv9.bias, dh9.shape[-1], dh9.device, exact_zero_bias)
    dw9, _ = ops.conv_wgrad(d9, s.a6, dh9, P.conv9.weight.shape, dw=o.conv9.weight, dbias=want9, want_bias=want9 is not None)
    da6 = ops.conv_dgrad(d9, dh9, wd9)
    da3, g6, g7 = _bn_relu_conv_backward(d6, wd6, s.a3, s.h6, da6, s.m7, s.i7, P.bn7, o.conv6, o.bn7, P.conv6.weight.shape, exact_zero_bias)
    da0, g3, g4 = _bn_relu_conv_backward(d3, wd3, s.a0, s.h3, da3, s.m4, s.i4, P.bn4, o.conv3, o.bn4, P.conv3.weight.shape, exact_zero_bias)
    if s.h0 is None:
        dw0, db0, dg1, dbe1 = ops.c1conv_bn_relu_backward(s.x, P.conv0.weight, P.conv0.bias, P.bn1.weight, P.bn1.bias, s.m1, s.i1, da0,
                                                          dw=o.conv0.weight, dbias=o.conv0.bias, dgamma=o.bn1.weight, dbeta=o.bn1.bias,
                                                          moments=s.mom0)
        if exact_zero_bias:
            db0.zero_()
        g0, g1 = LayerGrads(dw0, db0), LayerGrads(dg1, dbe1)
    else:
        _, g0, g1 = _bn_relu_conv_backward(d0, None, s.x, s.h0, da0, s.m1, s.i1, P.bn1, o.conv0, o.bn1, P.conv0.weight.shape, exact_zero_bias,
                                           need_dx=False)
    return VAEEncoderGrads(conv0=g0, bn1=g1, conv3=g3, bn4=g4, conv6=g6, bn7=g7, conv9=LayerGrads(dw9, db9), bn10=bn10)


# ------------------------------------------------------------------------------------------------
# The Gaussian latent   (src/models.py:77,104-114)
# ------------------------------------------------------------------------------------------------
def latent_forward(h9, m10, i10, bn10: BNParams, eps):
    """-> (z NHWC (B, 14, w, Z), kl [1]); eps NHWC like z."""
    return ops.vae_latent_forward(h9, m10, i10, bn10.weight, bn10.bias, eps)


def latent_backward(dz, h9, m10, i10, bn10: BNParams, eps, kl_scale=1.0, kl_grad=None, gout: Optional[LayerGrads] = None):
    """-> (dh9, encoder.10's LayerGrads).  Training-mode statistics: the BatchNorm's backward is finished by bn_backward_apply
    from the sums the latent kernel formed while it wrote dy."""
    o = gout if gout is not None else LayerGrads()
    dy, dg, dbe = ops.vae_latent_backward(h9, m10, i10, bn10.weight, bn10.bias, eps, dz, kl_scale=kl_scale, kl_grad=kl_grad,
                                          dgamma=o.weight, dbeta=o.bias)
    return ops.bn_backward_apply(h9, dy, m10, i10, bn10.weight, dg, dbe), LayerGrads(dg, dbe)


# ------------------------------------------------------------------------------------------------
# Decoder   (src/models.py:81-93)
# ------------------------------------------------------------------------------------------------
class VAEDecoderSaved(NamedTuple):
    """z the latent sample; u0, u3, u6 the transposed convs' outputs; a1, a4, a7 the activated tensors; xt the image."""
    z: torch.Tensor
    u0: torch.Tensor
    a1: torch.Tensor
    m1: torch.Tensor
    i1: torch.Tensor
    u3: torch.Tensor
    a4: torch.Tensor
    m4: torch.Tensor
    i4: torch.Tensor
    u6: torch.Tensor
    a7: torch.Tensor
    m7: torch.Tensor
    i7: torch.Tensor
    xt: torch.Tensor
    d: tuple
    wd: tuple


def decoder_forward(z, P: VAEDecoderParams, training: bool, packs=None):
    """z fp32 NHWC (B, 14, w, Z) -> (x_tilde fp32 NHWC (B, 80, 4 (w + 6), 1), saved)."""
    B, h, w, Z = z.shape
    D = P.convt0.weight.shape[1]
    t0, t3, t6, t9 = _decoder_descs(B, h, w, D, Z)
    wf0, wd0 = _pack(packs, "convt0", t0, P.convt0)
    u0, m1, i1 = _conv_bn(t0, z, wf0, P.convt0, P.bn1, training)
    a1 = ops.bn_apply(u0, m1, i1, P.bn1.weight, P.bn1.bias, relu=True)
    wf3, wd3 = _pack(packs, "convt3", t3, P.convt3)
    u3, m4, i4 = _conv_bn(t3, a1, wf3, P.convt3, P.bn4, training)
    a4 = ops.bn_apply(u3, m4, i4, P.bn4.weight, P.bn4.bias, relu=True)
    wf6, wd6 = _pack(packs, "convt6", t6, P.convt6)
    u6, m7, i7 = _conv_bn(t6, a4, wf6, P.convt6, P.bn7, training)
    a7 = ops.bn_apply(u6, m7, i7, P.bn7.weight, P.bn7.bias, relu=True)
    wf9, wd9 = _pack(packs, "convt9", t9, P.convt9)
    xt = ops.conv_forward(t9, a7, wf9, P.convt9.bias, flags=NSG_TANH_OUT)
    return xt, VAEDecoderSaved(z, u0, a1, m1, i1, u3, a4, m4, i4, u6, a7, m7, i7, xt, (t0, t3, t6, t9), (wd0, wd3, wd6, wd9))


def decoder_backward(dxt, saved: VAEDecoderSaved, P: VAEDecoderParams, need_dz: bool = True, dxt_is_pre_tanh: bool = False,
                     gout: Optional[VAEDecoderGrads] = None, exact_zero_bias: bool = False):
    """dxt: the gradient at x_tilde (or at the Tanh's input when dxt_is_pre_tanh) -> (dz or None, VAEDecoderGrads)."""
    s = saved
    o = gout if gout is not None else VAEDecoderGrads()
    t0, t3, t6, t9 = s.d
    wd0, wd3, wd6, wd9 = s.wd
    dpre = dxt if dxt_is_pre_tanh else ops.tanh_backward(dxt, s.xt)
    dw9, db9 = ops.conv_wgrad(t9, s.a7, dpre, P.convt9.weight.shape, dw=o.convt9.weight, dbias=o.convt9.bias)
    da7 = ops.conv_dgrad(t9, dpre, wd9)
    da4, g6, g7 = _bn_relu_conv_backward(t6, wd6, s.a4, s.u6, da7, s.m7, s.i7, P.bn7, o.convt6, o.bn7, P.convt6.weight.shape, exact_zero_bias)
    da1, g3, g4 = _bn_relu_conv_backward(t3, wd3, s.a1, s.u3, da4, s.m4, s.i4, P.bn4, o.convt3, o.bn4, P.convt3.weight.shape, exact_zero_bias)
    dz, g0, g1 = _bn_relu_conv_backward(t0, wd0, s.z, s.u0, da1, s.m1, s.i1, P.bn1, o.convt0, o.bn1, P.convt0.weight.shape, exact_zero_bias,
                                        need_dx=need_dz)
    return dz, VAEDecoderGrads(convt0=g0, bn1=g1, convt3=g3, bn4=g4, convt6=g6, bn7=g7, convt9=LayerGrads(dw9, db9))


# ------------------------------------------------------------------------------------------------
# parameter bundles out of the nn.Module tree; records <-> lists of tensors in state_dict order
# ------------------------------------------------------------------------------------------------
def encoder_params(enc) -> VAEEncoderParams:
    return VAEEncoderParams(conv_params(enc[0]), bn_params(enc[1]), conv_params(enc[3]), bn_params(enc[4]), conv_params(enc[6]),
                            bn_params(enc[7]), conv_params(enc[9]), bn_params(enc[10]))


def decoder_params(dec) -> VAEDecoderParams:
    return VAEDecoderParams(conv_params(dec[0]), bn_params(dec[1]), conv_params(dec[3]), bn_params(dec[4]), conv_params(dec[6]),
                            bn_params(dec[7]), conv_params(dec[9]))


def encoder_param_list(P: VAEEncoderParams) -> List[torch.Tensor]:
    return _flatten(P, VAE_ENCODER_LAYERS)


def decoder_param_list(P: VAEDecoderParams) -> List[torch.Tensor]:
    return _flatten(P, VAE_DECODER_LAYERS)


def encoder_grad_list(g: VAEEncoderGrads) -> List[torch.Tensor]:
    return _flatten(g, VAE_ENCODER_LAYERS)


def decoder_grad_list(g: VAEDecoderGrads) -> List[torch.Tensor]:
    return _flatten(g, VAE_DECODER_LAYERS)


def encoder_grads(tensors) -> VAEEncoderGrads:
    return _bind(VAEEncoderGrads(), VAE_ENCODER_LAYERS, tensors)


def decoder_grads(tensors) -> VAEDecoderGrads:
    return _bind(VAEDecoderGrads(), VAE_DECODER_LAYERS, tensors)
