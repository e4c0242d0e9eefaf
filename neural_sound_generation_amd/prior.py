"""The latent prior of the model family: the reference's GatedPixelCNN over the grid of code indices
(src/models.py:219-341), on the HIP kernels of the main path.

Same class names, constructor arguments, attributes and state_dict keys as the reference (GatedActivation,
GatedMaskedConv2d, GatedPixelCNN), same initialisation (identical RNG consumption: `torch.manual_seed(s);
GatedPixelCNN(...)` reproduces the reference's initial weights bit for bit, tests/test_host_logic.py).

How it maps onto the kernels:
  * every convolution is nsg_conv_forward / nsg_conv_dgrad / nsg_conv_wgrad.  The masked stacks use rectangular kernels
    with pad-then-crop -- vertical (k//2+1, k) padded (k//2, k//2) and cropped to H rows, horizontal (1, k//2+1) padded
    (0, k//2) and cropped to W columns (models.py:238-252,268-273): the conv descriptor's rectangular form (k, k_w, pad,
    pad_w, cropped OH / OW), so only the taps that exist are computed;
  * GatedActivation with the class-conditional add is one kernel each way (nsg_gated_activation_*);
  * the two embeddings are nsg_gather_rows / nsg_index_add_rows; the cross-entropy of the logits is nsg_cross_entropy.
All tensors between kernels are fp32 NHWC rows; module inputs / outputs keep the reference's NCHW logical shapes
(channels_last views).

One deliberate generalisation (also in oracle/pixelcnn_oracle.py): the reference crops the vertical stack's rows with the
input WIDTH and the horizontal stack's columns with the input HEIGHT (models.py:269,273), so it only runs on square grids;
here rows are cropped to the height and columns to the width -- identical on square grids, and what the (20, T/4) grid of
the VQ-VAE's codes needs.  `generate` is the evident intent of the reference's (which passes a nested tuple to
torch.zeros, models.py:325-341).
"""
from __future__ import annotations

import math
import numbers

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import functional as Fn, ops
from .models import weights_init
from .vector_quantization import codebook_lookup


class _Conv(Function):
    """y = conv2d(x, w, b) on NHWC rows, stride 1, kernel (kh, kw) = w's own extent, padding (ph, pw), the output cropped to
    the input's (H, W) at the bottom / right -- the reference's pad-then-crop of the masked stacks (models.py:268-273) and,
    for odd square kernels with pad = k // 2, plain 'same' convolution.  Optional ReLU of the output."""

    @staticmethod
    def forward(ctx, x, w, b, pad, relu_out):
        x = x.contiguous()
        B, H, W, Ci = x.shape
        Co, _, kh, kw = w.shape
        d = ops.conv_desc(B, H, W, Ci, Co, (kh, kw), 1, pad, out_hw=(H, W))
        wf, wd = ops.pack_weights(d, w.detach().contiguous())
        y = ops.conv_forward(d, x, wf, b.detach(), flags=ops.NSG_RELU_OUT if relu_out else 0)
        ctx.d, ctx.wd, ctx.relu_out, ctx.wshape = d, wd, relu_out, tuple(w.shape)
        ctx.save_for_backward(x, y if relu_out else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        gy = gy.contiguous()
        if ctx.relu_out:
            gy = ops.relu_backward_add(gy, None, y)
        dw, db = ops.conv_wgrad(ctx.d, x, gy, ctx.wshape)
        dx = ops.conv_dgrad(ctx.d, gy, ctx.wd) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None, None


class _Gate(Function):
    """tanh(a) * sigmoid(b) of the channel halves of x (+ per-clip conditioning rows)."""

    @staticmethod
    def forward(ctx, x, cond):
        x = x.contiguous()
        cond = cond.contiguous() if cond is not None else None
        ctx.save_for_backward(x, cond)
        return ops.gated_activation(x, cond)

    @staticmethod
    def backward(ctx, gy):
        x, cond = ctx.saved_tensors
        dx = ops.gated_activation_backward(x, cond, gy.contiguous())
        dcond = ops.clip_colsum(dx, cond.shape[0]) if (cond is not None and ctx.needs_input_grad[1]) else None
        return dx, dcond


class _Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, g


class _CrossEntropy(Function):
    @staticmethod
    def forward(ctx, logits2d, target):
        loss, dl = ops.cross_entropy(logits2d.contiguous(), target.contiguous(), want_grad=True)
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None


class _CrossEntropyMasked(Function):
    """Mean cross-entropy over the rows whose target is >= 0 (nsg_cross_entropy_masked); clips of rows_per_clip rows."""

    @staticmethod
    def forward(ctx, logits2d, target, rows_per_clip):
        loss, dl, _, _ = ops.cross_entropy_masked(logits2d.contiguous(), target.contiguous(), rows_per_clip, want_grad=True)
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None


def masked_targets(x, lengths):
    """x int64 (B, H, W), lengths int64 (B,) = valid columns per clip -> the loss targets (B, H, W): x where the column is
    < lengths[b], -1 (ignored) elsewhere.  Built on x's device, no host synchronisation."""
    W = x.shape[-1]
    valid = torch.arange(W, device=x.device)[None, None, :] < lengths.to(x.device)[:, None, None]
    return torch.where(valid, x, torch.full_like(x, -1))


def _conv(x_nhwc, conv: nn.Conv2d, relu_out: bool = False):
    """The module's own (possibly rectangular) kernel and padding, output cropped to the input extent."""
    return _Conv.apply(x_nhwc, conv.weight, conv.bias, tuple(conv.padding), relu_out)


class GatedActivation(nn.Module):
    def forward(self, x):
        return Fn.to_nchw_view(_Gate.apply(Fn.to_nhwc(x), None))


class GatedMaskedConv2d(nn.Module):
    def __init__(self, mask_type, dim, kernel, residual=True, n_classes=10):
        super().__init__()
        assert kernel % 2 == 1, "Kernel size must be odd"
        self.mask_type = mask_type
        self.residual = residual
        self.kernel = kernel
        self.class_cond_embedding = nn.Embedding(n_classes, 2 * dim)
        self.vert_stack = nn.Conv2d(dim, dim * 2, (kernel // 2 + 1, kernel), 1, (kernel // 2, kernel // 2))
        self.vert_to_horiz = nn.Conv2d(2 * dim, 2 * dim, 1)
        self.horiz_stack = nn.Conv2d(dim, dim * 2, (1, kernel // 2 + 1), 1, (0, kernel // 2))
        self.horiz_resid = nn.Conv2d(dim, dim, 1)
        self.gate = GatedActivation()

    def make_causal(self):
        self.vert_stack.weight.data[:, :, -1].zero_()       # mask the final row
        self.horiz_stack.weight.data[:, :, :, -1].zero_()   # mask the final column

    def forward_nhwc(self, x_v, x_h, h):
        """x_v, x_h (B, H, W, dim) NHWC rows, h (B,) int64 class labels -> (out_v, out_h) NHWC."""
        if self.mask_type == 'A':
            self.make_causal()
        cond = codebook_lookup(self.class_cond_embedding.weight, h.view(-1))          # (B, 2 dim)
        h_vert = _conv(x_v, self.vert_stack)
        out_v = _Gate.apply(h_vert, cond)
        h_horiz = _conv(x_h, self.horiz_stack)
        v2h = _conv(h_vert, self.vert_to_horiz)
        out = _Gate.apply(_Add.apply(v2h, h_horiz), cond)
        out_h = _conv(out, self.horiz_resid)
        if self.residual:
            out_h = _Add.apply(out_h, x_h)
        return out_v, out_h

    def forward(self, x_v, x_h, h):
        out_v, out_h = self.forward_nhwc(Fn.to_nhwc(x_v), Fn.to_nhwc(x_h), h)
        return Fn.to_nchw_view(out_v), Fn.to_nchw_view(out_h)


class GatedPixelCNN(nn.Module):
    def __init__(self, input_dim=256, dim=64, n_layers=15, n_classes=10):
        super().__init__()
        if dim % 4 != 0:
            raise ValueError("GatedPixelCNN: dim must be a multiple of 4 on this path")
        self.dim = dim
        self.embedding = nn.Embedding(input_dim, dim)
        self.layers = nn.ModuleList()
        for i in range(n_layers):
            mask_type = 'A' if i == 0 else 'B'
            kernel = 7 if i == 0 else 3
            residual = False if i == 0 else True
            self.layers.append(GatedMaskedConv2d(mask_type, dim, kernel, residual, n_classes))
        self.output_conv = nn.Sequential(nn.Conv2d(dim, 512, 1), nn.ReLU(True), nn.Conv2d(512, input_dim, 1))
        self.apply(_weights_init_quiet)

    def forward_nhwc(self, x, label):
        """x int64 (B, H, W), label int64 (B,) -> logits (B, H, W, input_dim) NHWC rows."""
        B, H, W = x.shape
        e = codebook_lookup(self.embedding.weight, x.reshape(-1)).view(B, H, W, self.dim)
        x_v, x_h = e, e
        for layer in self.layers:
            x_v, x_h = layer.forward_nhwc(x_v, x_h, label)
        y = _conv(x_h, self.output_conv[0], relu_out=True)     # the ReLU is fused into the conv's store
        return _conv(y, self.output_conv[2])

    def forward(self, x, label):
        return Fn.to_nchw_view(self.forward_nhwc(x, label))

    def loss(self, x, label, lengths=None):
        """Mean cross-entropy of the prior's logits against the codes themselves (each code from its causal context).
        lengths int64 (B,): valid latent columns per clip, 0 <= lengths[b] <= W; the positions [b, :, lengths[b]:] (the padding
        of a zero-padded batch) are left out of the mean.  No valid position at all gives 0 (not NaN).  The codes under the
        padding still lie in the causal context of valid positions of later rows: nothing is masked on the input side."""
        if lengths is None:
            logits = self.forward_nhwc(x, label)
            return _CrossEntropy.apply(logits.view(-1, logits.shape[-1]), x.reshape(-1))
        x, label, lengths = self.check_batch(x, label, lengths)
        logits = self.forward_nhwc(x, label)
        return _CrossEntropyMasked.apply(logits.view(-1, logits.shape[-1]), masked_targets(x, lengths).reshape(-1), x.shape[1] * x.shape[2])

    @torch.no_grad()
    def nll(self, x, label, lengths=None):
        """Each clip's summed negative log-likelihood in nats over its valid positions, and their number:
        (nll (B,) fp32, count (B,) int64).  lengths as in `loss` (None: every position is valid)."""
        x, label, lengths = self.check_batch(x, label, lengths)
        logits = self.forward_nhwc(x, label)
        target = x if lengths is None else masked_targets(x, lengths)
        _, _, nll, count = ops.cross_entropy_masked(logits.view(-1, logits.shape[-1]), target.reshape(-1).contiguous(), x.shape[1] * x.shape[2],
                                                    want_grad=False, want_clip=True)
        return nll, count

    def check_batch(self, x, label, lengths=None):
        """Validates a training batch (ValueError) and returns it on the model's device: codes int64 (B, H, W), label int64 (B,)
        in [0, n_classes), lengths None or int64 (B,) in [0, W].  The value checks read the tensors where they are: free for
        host tensors (what a loader yields), one synchronisation for device tensors."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.int64:
            raise ValueError("codes must be an int64 tensor (B, H, W)")
        B, H, W = x.shape
        self._grid((H, W))
        label = self._labels(label, B)
        if lengths is not None:
            if not isinstance(lengths, torch.Tensor) or tuple(lengths.shape) != (B,) or lengths.dtype != torch.int64:
                raise ValueError(f"lengths must be an int64 tensor of shape ({B},)")
            if int(lengths.min()) < 0 or int(lengths.max()) > W:
                raise ValueError(f"lengths outside [0, {W}]")
            lengths = lengths.to(label.device).contiguous()
        return x.to(label.device).contiguous(), label, lengths

    @torch.no_grad()
    def generate(self, label, shape=(8, 8), batch_size=64):
        """Ancestral sampling in raster order (the intent of models.py:325-341)."""
        param = next(self.parameters())
        x = torch.zeros((batch_size,) + tuple(shape), dtype=torch.int64, device=param.device)
        for i in range(shape[0]):
            for j in range(shape[1]):
                logits = self.forward_nhwc(x, label)
                probs = F.softmax(logits[:, i, j, :], -1)
                x[:, i, j] = probs.multinomial(1).squeeze(-1)
        return x

    # ------------------------------------------------------------------------------------------------
    # incremental sampling: one row pass (conv kernels) and one column walk (nsg_prior_walk) per row
    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, label, shape=(8, 8), batch_size=64, u=None, generator=None, *, temperature=1.0, top_k=0, top_p=1.0,
               given=None, keep=None, guidance=0.0, null_label=None):
        """Ancestral sampling in raster order with nothing recomputed: int64 codes (batch_size, H, W).  Each code is the
        inverse CDF of its softmax against u[b, i, j] (include/nsg.h, nsg_prior_walk); u is drawn with torch.rand on the
        model's device when not given.  The same distribution as `generate`, O(H W) work instead of O((H W)^2).

        Controls of the pick (include/nsg.h, nsg_prior_walk_ctl, states the exact rule): temperature > 0 divides the logits;
        top_k >= 1 keeps the top_k largest logits (ties kept; 0 or >= input_dim: off); top_p < 1 keeps the smallest set of
        most probable codes whose mass reaches top_p (ties kept; 1: off).  With all three off and nothing given this is the
        plain walk, and its results do not move.

        Priming: given int64 (B, H, W) and keep bool (B, H, W) come together; where keep is set the result holds given's code
        and only the other positions are sampled.  This is not posterior inference: each sampled code is drawn from the
        prior's conditional given everything BEFORE it in raster order, kept or sampled, and kept codes later in raster order
        do not influence it.  Keeping whole leading rows is exact conditional sampling; keeping the first columns of every
        row is the usual "hold the known, sample the rest".

        Classifier-free guidance (include/nsg.h, nsg_prior_walk_cfg): with guidance > 0, a real number up to 1024, every
        clip is walked twice, under its label and under null_label (an integer in [0, n_classes), required then and refused
        otherwise), and each code is picked -- by the controls above, against the same u -- from the logits
        l_c + guidance * (l_c - l_u); both branches continue from that code.  It pushes a sample towards what its label
        adds over the null class, which is something only for a prior trained with label dropout on that null class
        (prior_train.drop_labels).  guidance == 0 is the sampler without it: the same launches, the same bits."""
        H, W = self._grid(shape)
        B = int(batch_size)
        label = self._labels(label, B)
        dev = label.device
        ctl = self._controls(temperature, top_k, top_p)
        guided = self._guidance(guidance, null_label)
        if (given is None) != (keep is None):
            raise ValueError("sample: given and keep come together")
        if given is not None:
            if not isinstance(given, torch.Tensor) or tuple(given.shape) != (B, H, W) or given.dtype != torch.int64:
                raise ValueError(f"sample: given must be an int64 tensor of shape {(B, H, W)}")
            if not isinstance(keep, torch.Tensor) or tuple(keep.shape) != (B, H, W) or keep.dtype != torch.bool:
                raise ValueError(f"sample: keep must be a bool tensor of shape {(B, H, W)}")
            given, keep = given.to(dev).contiguous(), keep.to(dev).contiguous()
            kept = given[keep]
            K = self.embedding.num_embeddings
            if kept.numel() and (int(kept.min()) < 0 or int(kept.max()) >= K):
                raise ValueError(f"sample: kept codes outside [0, {K})")
        if u is None:
            self._check_walk()
            u = torch.rand((B, H, W), generator=generator, device=dev)
        elif not isinstance(u, torch.Tensor) or tuple(u.shape) != (B, H, W) or u.dtype != torch.float32:
            raise ValueError(f"sample: u must be a float32 tensor of shape {(B, H, W)}")
        codes = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        if guided is not None:                       # 2B clips: [label[0], null, label[1], null, ...]; u, given, keep and codes per pair
            pairs = torch.stack([label, torch.full_like(label, guided[1])], 1).reshape(-1)
            self._walk_rows(pairs, 2 * B, H, W, u=u.to(dev).contiguous(), codes=codes, x_in=given, keep=keep, ctl=ctl or (1.0, 0, 1.0),
                            guidance=guided[0])
        elif ctl is None and given is None:
            self._walk_rows(label, B, H, W, u=u.to(dev).contiguous(), codes=codes)
        else:
            self._walk_rows(label, B, H, W, u=u.to(dev).contiguous(), codes=codes, x_in=given, keep=keep, ctl=ctl or (1.0, 0, 1.0))
        return codes

    @torch.no_grad()
    def continue_codes(self, prefix, label, width, **controls):
        """Continue a grid of codes in time: prefix int64 (B, H, W0) with W0 <= width -> int64 (B, H, width) whose columns
        < W0 are the prefix and whose other columns are sampled (`sample` with the first W0 columns of every row kept;
        controls: sample's u, generator, temperature, top_k, top_p, guidance, null_label).  Not posterior inference: a sampled code is conditioned
        on what precedes it in raster order -- the rows above, prefix and continuation, and its own row to its left -- and
        not on the prefix columns of the rows below it."""
        if not isinstance(prefix, torch.Tensor) or prefix.dim() != 3 or prefix.dtype != torch.int64:
            raise ValueError("continue_codes: prefix must be an int64 tensor (B, H, W0)")
        B, H, W0 = prefix.shape
        width = int(width)
        if W0 > width:
            raise ValueError(f"continue_codes: the prefix has {W0} columns, more than width = {width}")
        given = torch.zeros((B, H, width), dtype=torch.int64, device=prefix.device)
        given[:, :, :W0] = prefix
        keep = torch.zeros((B, H, width), dtype=torch.bool, device=prefix.device)
        keep[:, :, :W0] = True
        return self.sample(label, shape=(H, width), batch_size=B, given=given, keep=keep, **controls)

    def _controls(self, temperature, top_k, top_p):
        """Validates the pick's controls; None when all three are off (the plain walk), else (temperature, top_k, top_p)."""
        K = self.embedding.num_embeddings
        for v, nm in ((temperature, "temperature"), (top_p, "top_p")):
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError(f"sample: {nm} must be a number")
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or top_k < 0:
            raise ValueError("sample: top_k must be an integer >= 0 (0: off)")
        inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(temperature), dtype=torch.float32)
        if not (math.isfinite(temperature) and temperature > 0 and bool(torch.isfinite(inv_t))):
            raise ValueError("sample: temperature must be finite and > 0 (and so must its fp32 reciprocal)")
        if not 0 < top_p <= 1:
            raise ValueError("sample: top_p must be in (0, 1] (1: off)")
        top_k = 0 if top_k >= K else int(top_k)
        if float(temperature) == 1.0 and top_k == 0 and float(top_p) == 1.0:
            return None
        return float(temperature), top_k, float(top_p)

    def _guidance(self, guidance, null_label):
        """Validates sample's guidance and null_label; None without guidance, else (guidance, null_label)."""
        if isinstance(guidance, bool) or not isinstance(guidance, numbers.Real):
            raise ValueError("sample: guidance must be a number")
        if not 0 <= guidance <= 1024:                # NaN fails both comparisons
            raise ValueError("sample: guidance must be in [0, 1024] (0: off)")
        if guidance == 0:
            if null_label is not None:
                raise ValueError("sample: null_label is given without guidance")
            return None
        n_classes = self.layers[0].class_cond_embedding.num_embeddings
        if null_label is None or isinstance(null_label, bool) or not isinstance(null_label, numbers.Integral):
            raise ValueError("sample: guidance > 0 needs null_label, an integer class")
        if not 0 <= null_label < n_classes:
            raise ValueError(f"sample: null_label outside [0, {n_classes})")
        return float(guidance), int(null_label)

    @torch.no_grad()
    def incremental_logits(self, x, label):
        """Teacher-forced logits (B, H, W, input_dim) NHWC of the codes x (B, H, W) through the sampling schedule: what
        forward_nhwc computes, one row pass and one column walk per row."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.int64:
            raise ValueError("incremental_logits: x must be an int64 tensor (B, H, W)")
        B, H, W = x.shape
        self._grid((H, W))
        label = self._labels(label, B)
        x = x.to(label.device).contiguous()
        K = self.embedding.num_embeddings
        if x.numel() and (int(x.min()) < 0 or int(x.max()) >= K):
            raise ValueError(f"incremental_logits: codes outside [0, {K})")
        logits = torch.empty((B, H, W, K), dtype=torch.float32, device=x.device)
        self._walk_rows(label, B, H, W, x_in=x, logits=logits)
        return logits

    def walk_supported(self) -> bool:
        """Whether sample / incremental_logits run for this module's widths (generate serves every width)."""
        oc = self.output_conv
        return oc[0].out_channels == 512 and ops.prior_walk_weight_floats(self.dim, len(self.layers), self.embedding.num_embeddings) > 0

    def _check_walk(self):
        if not self.walk_supported():
            raise NotImplementedError(f"GatedPixelCNN(input_dim={self.embedding.num_embeddings}, dim={self.dim}, n_layers={len(self.layers)}): "
                                      "outside the incremental sampler's envelope (dim % 16 == 0, dim <= 128, input_dim <= 1024); "
                                      "use generate()")

    @staticmethod
    def _grid(shape):
        if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
            raise ValueError(f"the code grid {tuple(shape)} must be (H, W) with H, W >= 1")
        return int(shape[0]), int(shape[1])

    def _labels(self, label, B):
        if B < 1:
            raise ValueError("batch_size must be at least 1")
        if not isinstance(label, torch.Tensor) or tuple(label.shape) != (B,) or label.dtype != torch.int64:
            raise ValueError(f"label must be an int64 tensor of shape ({B},)")
        n_classes = self.layers[0].class_cond_embedding.num_embeddings
        label = label.to(next(self.parameters()).device).contiguous()
        if int(label.min()) < 0 or int(label.max()) >= n_classes:
            raise ValueError(f"label values outside [0, {n_classes})")
        return label

    def _walk_blob(self, K):
        """The walk's packed weights (include/nsg.h, nsg_prior_walk): every matrix transposed to input-major."""
        parts = []
        for i, layer in enumerate(self.layers):
            taps = 3 if i == 0 else 2                                 # layer 0's fourth tap (column j) is masked
            hw = layer.horiz_stack.weight.detach()[:, :, 0, :taps]    # (2 dim, dim, taps)
            parts += [hw.permute(2, 1, 0).reshape(-1), layer.horiz_stack.bias.detach(),
                      layer.horiz_resid.weight.detach()[:, :, 0, 0].t().reshape(-1), layer.horiz_resid.bias.detach()]
        w0, w2 = self.output_conv[0], self.output_conv[2]
        Kp = (K + 3) // 4 * 4
        w2t = torch.zeros(512, Kp, dtype=torch.float32, device=w2.weight.device)
        w2t[:, :K] = w2.weight.detach()[:, :, 0, 0].t()
        b2 = torch.zeros(Kp, dtype=torch.float32, device=w2.weight.device)
        b2[:K] = w2.bias.detach()
        parts += [w0.weight.detach()[:, :, 0, 0].t().reshape(-1), w0.bias.detach(), w2t.reshape(-1), b2]
        return torch.cat([p.reshape(-1).float() for p in parts]).contiguous()

    def _walk_rows(self, label, B, H, W, u=None, codes=None, x_in=None, logits=None, times=None, ctl=None, keep=None, guidance=None):
        """Row i: the row pass (vertical stacks, their gates and the v2h 1x1s of every layer, all W columns, on the conv
        kernels), then the column walk.  Layer 0 reads rows i-3 .. i of e (row i is masked: zeros until the walk writes it),
        the others rows i-1, i of their vertical input; rows above the grid are zero, as the conv's padding is.
        times: optional dict that collects the row passes' and walks' GPU milliseconds (scripts/prior_sample_timing.py).
        ctl: None for the plain walk (nsg_prior_walk), or (temperature, top_k, top_p) for the controlled one
        (nsg_prior_walk_ctl), which also takes keep (B, H, W) with x_in as the kept codes.
        guidance: None, or with ctl the guided walk (nsg_prior_walk_cfg): B = 2P clips whose labels interleave each pair's
        real and null label, while u, codes, x_in and keep are (P, H, W); logits stays (B, H, W, K).  The row pass is the
        same one on the 2P clips."""
        self._check_walk()
        self.layers[0].make_causal()
        dim, L, K = self.dim, len(self.layers), self.embedding.num_embeddings
        dev = label.device
        blob = self._walk_blob(K)
        emb = self.embedding.weight.detach().contiguous()
        cond = torch.stack([ops.gather_rows(layer.class_cond_embedding.weight.detach().contiguous(), label) for layer in self.layers])
        d0 = ops.conv_desc(B, 4, W, dim, 2 * dim, (4, 7), 1, (0, 3), out_hw=(1, W))
        dv = ops.conv_desc(B, 2, W, dim, 2 * dim, (2, 3), 1, (0, 1), out_hw=(1, W))
        d11 = ops.conv_desc(B, 1, W, 2 * dim, 2 * dim, 1, 1, 0, out_hw=(1, W))
        # Layer l >= 1 keeps rows i-1, i of its vertical input in a 2-row strip, row i in slot i % 2: on even rows the slots
        # are in reverse order, which the same kernel with its two rows swapped reads in place (no shift copy).
        vw = [layer.vert_stack.weight.detach().contiguous() for layer in self.layers]
        jobs = [(d0, vw[0], True, False)] + [(dv, w, True, False) for w in vw[1:]] + [(dv, w.flip(2).contiguous(), True, False) for w in vw[1:]]
        jobs += [(d11, layer.vert_to_horiz.weight.detach().contiguous(), True, False) for layer in self.layers]
        packed = [wf for wf, _ in ops.pack_weights_batch(jobs)]
        vert_w, vert_w_flip, v2h_w = packed[:L], [None] + packed[L:2 * L - 1], packed[2 * L - 1:]
        e_grid = torch.zeros((B, H + 3, W, dim), dtype=torch.float32, device=dev)   # e with 3 zero rows above the grid
        e_strip = torch.empty((B, 4, W, dim), dtype=torch.float32, device=dev)
        strips = torch.zeros((L, B, 2, W, dim), dtype=torch.float32, device=dev)     # slot i % 2: row i of layer l's vertical input
        h_vert = torch.empty((L, B, 1, W, 2 * dim), dtype=torch.float32, device=dev)
        v = torch.empty((B, 1, W, dim), dtype=torch.float32, device=dev)
        vh = torch.empty((L, B, 1, W, 2 * dim), dtype=torch.float32, device=dev)
        vert, v2h, gate = [], [], []
        for l, layer in enumerate(self.layers):
            vb = layer.vert_stack.bias.detach()
            if l == 0:
                vert.append((ops.prepared_conv_forward(d0, e_strip, vert_w[0], vb, h_vert[0]),) * 2)
            else:
                vert.append((ops.prepared_conv_forward(dv, strips[l], vert_w_flip[l], vb, h_vert[l]),     # even rows
                             ops.prepared_conv_forward(dv, strips[l], vert_w[l], vb, h_vert[l])))         # odd rows
            v2h.append(ops.prepared_conv_forward(d11, h_vert[l], v2h_w[l], layer.vert_to_horiz.bias.detach(), vh[l]))
            gate.append(ops.prepared_gated_activation(h_vert[l], cond[l], v) if l + 1 < L else None)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if times is not None else None
        for i in range(H):
            if ev:
                ev[0].record()
            e_strip.copy_(e_grid[:, i:i + 4])
            for l in range(L):
                vert[l][i % 2]()
                if gate[l] is not None:
                    gate[l]()
                    strips[l + 1, :, i % 2].copy_(v[:, 0])
                v2h[l]()
            if ev:
                ev[1].record()
            if guidance is not None:
                ops.prior_walk_cfg(blob, emb, cond, vh, e_grid[:, i + 3], H, i, u, codes, guidance, x_in=x_in, keep=keep, logits=logits,
                                   temperature=ctl[0], top_k=ctl[1], top_p=ctl[2])
            elif ctl is None:
                ops.prior_walk(blob, emb, cond, vh, e_grid[:, i + 3], H, i, u=u, x_in=x_in, codes=codes, logits=logits)
            else:
                ops.prior_walk_ctl(blob, emb, cond, vh, e_grid[:, i + 3], H, i, u, codes, x_in=x_in, keep=keep, logits=logits,
                                   temperature=ctl[0], top_k=ctl[1], top_p=ctl[2])
            if ev:
                ev[2].record()
                ev[2].synchronize()
                times["row_pass_ms"] = times.get("row_pass_ms", 0.0) + ev[0].elapsed_time(ev[1])
                times["walk_ms"] = times.get("walk_ms", 0.0) + ev[1].elapsed_time(ev[2])


def _weights_init_quiet(m):
    """models.weights_init (src/models.py:25-32) without the reference's "Skipping initialization of ..." print for the
    gated layers (their class name contains 'Conv' but they own no .weight: the reference skips them too)."""
    if isinstance(m, GatedMaskedConv2d):
        return
    weights_init(m)
