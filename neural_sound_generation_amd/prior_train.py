"""Stage two of the model family: training the latent prior (GatedPixelCNN) on the codes of a trained VQ-VAE.

  * `PriorTrainStep` -- the prior's counterpart of train.FusedTrainStep: one training step with no autograd graph.  It calls
    ops.* layer by layer on buffers it owns and writes every gradient straight into FlatAdam's flat bucket:
      - all layers' weights are re-packed in ONE pack_weights_batch launch per step;
      - the gate of the horizontal stack reads its two summands itself (nsg_gated_activation_sum_*: the [M][2C] sum is never
        stored), and both gates' backward passes form the class-conditioning gradient (the per-clip column sums of dx)
        while dx is written;
      - every gradient sum at a fork rides in a data-gradient store (nsg_conv_dgrad_relu_add, add = ...):
            d h_vert = dgrad_v2h(.) + gate_bwd(.),   d x_h = dgrad_horiz(.) + d out_h (residual),
            d e      = dgrad_horiz0(.) + dgrad_vert0(.);
      - the head's ReLU is fused into the conv's store forward (NSG_RELU_OUT) and into the data gradient's store backward;
      - the last layer's out_v feeds nothing: neither its gate nor that gate's backward is computed, and its class embedding
        takes its gradient from the horizontal gate alone (what autograd yields);
      - the loss is nsg_cross_entropy_masked: positions under a clip's padding carry target -1 and are left out.
    The gradients lie in one flat bucket (`opt.flat_grad`), so data parallelism is one all-reduce of it (not wired here).
  * `train_prior(args, vqvae, prior, step_or_optimizer, train_loader, device, epoch)` -- one epoch over a loader of
    (x, y, c, g, input_lengths): codes from the frozen VQ-VAE (evaluate.codes_from_mels), label = g (zeros without speakers).
  * `drop_labels(label, p, null_label, generator)` -- label dropout, the training half of classifier-free guidance; train_prior
    applies it before either kind of step when args.label_dropout > 0.  PriorTrainStep knows nothing of it.
"""
from __future__ import annotations

import numbers

import torch

from . import ops
from .optim import FlatAdam
from .prior import GatedPixelCNN, masked_targets


class _Plan:
    """Descriptors and buffers of one (B, H, W) grid: allocated once, reused by every step on that grid."""

    def __init__(self, model: GatedPixelCNN, B, H, W, device):
        dim, K = model.dim, model.embedding.num_embeddings
        self.shape = (B, H, W)

        def desc(conv):
            Co, Ci, kh, kw = conv.weight.shape
            return ops.conv_desc(B, H, W, Ci, Co, (kh, kw), 1, tuple(conv.padding), out_hw=(H, W))

        def buf(c):
            return torch.empty((B, H, W, c), dtype=torch.float32, device=device)

        self.descs = [{n: desc(getattr(layer, n)) for n in ("vert_stack", "horiz_stack", "vert_to_horiz", "horiz_resid")}
                      for layer in model.layers]
        self.head = (desc(model.output_conv[0]), desc(model.output_conv[2]))
        L = len(model.layers)
        self.e = buf(dim)
        self.act = [dict(cond=torch.empty((B, 2 * dim), dtype=torch.float32, device=device), h_vert=buf(2 * dim), h_horiz=buf(2 * dim),
                         v2h=buf(2 * dim), out=buf(dim), out_v=buf(dim) if l + 1 < L else None, out_h=buf(dim)) for l in range(L)]
        hidden = model.output_conv[0].out_channels
        self.y, self.logits, self.dlogits, self.dy = buf(hidden), buf(K), buf(K), buf(hidden)
        # gradients in flight: one set, reused by every layer
        self.d_out, self.dx_sum, self.dx_v, self.d_hvert = buf(dim), buf(2 * dim), buf(2 * dim), buf(2 * dim)
        self.d_xh, self.d_xv = (buf(dim), buf(dim)), buf(dim)
        self.dcond = torch.empty((2 * B, 2 * dim), dtype=torch.float32, device=device)   # [horizontal gate | vertical gate]


class PriorTrainStep:
    def __init__(self, model: GatedPixelCNN, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, optimizer: FlatAdam | None = None):
        if not isinstance(model, GatedPixelCNN):
            raise TypeError("PriorTrainStep trains a GatedPixelCNN")
        if model.layers[0].residual:
            raise ValueError("PriorTrainStep: layer 0 shares one input between its stacks and is not residual")
        self.model = model
        self.opt = optimizer if optimizer is not None else FlatAdam(model.parameters(), lr=lr, betas=betas, eps=eps)
        g = self.opt.grads_for
        self.g_emb = g([model.embedding.weight])[0]
        self.g_cls = g([layer.class_cond_embedding.weight for layer in model.layers])
        self.convs = [{n: getattr(layer, n) for n in ("vert_stack", "horiz_stack", "vert_to_horiz", "horiz_resid")} for layer in model.layers]
        self.g_conv = [{n: g([c.weight, c.bias]) for n, c in convs.items()} for convs in self.convs]
        self.head = (model.output_conv[0], model.output_conv[2])
        self.g_head = [g([c.weight, c.bias]) for c in self.head]
        self._plan = None         # the buffers of the last grid seen (a loader's batches of another width replace them)

    def _plan_for(self, B, H, W, device):
        if self._plan is None or self._plan.shape != (B, H, W):
            self._plan = None     # release before allocating the next
            self._plan = _Plan(self.model, B, H, W, device)
        return self._plan

    @torch.no_grad()
    def forward_backward(self, codes, label, lengths=None, *, check: bool = True):
        """codes int64 (B, H, W), label int64 (B,), lengths int64 (B,) = valid latent columns per clip (None: all) -> the mean
        cross-entropy over the valid positions (device scalar; nothing here synchronises with the host when check is False).
        Gradients land in opt.flat_grad (every p.grad is a view of it).  check: validate label / lengths (ValueError); a
        caller that has validated them on the host already passes False."""
        model = self.model
        if check:
            codes, label, lengths = model.check_batch(codes, label, lengths)
        B, H, W = codes.shape
        M, dim, K = B * H * W, model.dim, model.embedding.num_embeddings
        n_classes = model.layers[0].class_cond_embedding.num_embeddings
        L = len(model.layers)
        P = self._plan_for(B, H, W, codes.device)
        target = (codes if lengths is None else masked_targets(codes, lengths)).reshape(-1)
        label2 = torch.cat([label, label])

        # ---- weights: layer 0's masked taps zeroed in the parameters, then ONE pack launch for every conv
        model.layers[0].make_causal()
        jobs, names = [], ("vert_stack", "horiz_stack", "vert_to_horiz", "horiz_resid")
        for l in range(L):
            jobs += [(P.descs[l][n], self.convs[l][n].weight.detach(), True, True) for n in names]
        jobs += [(P.head[i], self.head[i].weight.detach(), True, True) for i in range(2)]
        packed = ops.pack_weights_batch(jobs)
        pk = [dict(zip(names, packed[4 * l:4 * l + 4])) for l in range(L)]
        pk_head = packed[4 * L:]

        def fwd(l, n, x, out):
            return ops.conv_forward(P.descs[l][n], x, pk[l][n][0], self.convs[l][n].bias.detach(), out=out)

        def wgrad(l, n, x, dy):
            c, (gw, gb) = self.convs[l][n], self.g_conv[l][n]
            ops.conv_wgrad(P.descs[l][n], x, dy, tuple(c.weight.shape), dw=gw, dbias=gb)

        def dgrad(l, n, dy, out, add=None):
            return ops.conv_dgrad(P.descs[l][n], dy, pk[l][n][1], out=out, add=add)

        # ---- forward
        ops.gather_rows(model.embedding.weight.detach(), codes, out=P.e)
        x_v = x_h = P.e
        inputs = []
        for l, layer in enumerate(model.layers):
            A = P.act[l]
            inputs.append((x_v, x_h))
            ops.gather_rows(layer.class_cond_embedding.weight.detach(), label, out=A["cond"])
            fwd(l, "vert_stack", x_v, A["h_vert"])
            if A["out_v"] is not None:
                ops.gated_activation(A["h_vert"], A["cond"], out=A["out_v"])
            fwd(l, "horiz_stack", x_h, A["h_horiz"])
            fwd(l, "vert_to_horiz", A["h_vert"], A["v2h"])
            ops.gated_activation_sum(A["v2h"], A["h_horiz"], A["cond"], out=A["out"])
            fwd(l, "horiz_resid", A["out"], A["out_h"])
            if layer.residual:
                ops.add(A["out_h"], x_h, out=A["out_h"])
            x_v, x_h = A["out_v"], A["out_h"]
        ops.conv_forward(P.head[0], x_h, pk_head[0][0], self.head[0].bias.detach(), flags=ops.NSG_RELU_OUT, out=P.y)
        ops.conv_forward(P.head[1], P.y, pk_head[1][0], self.head[1].bias.detach(), out=P.logits)
        loss, _, _, _ = ops.cross_entropy_masked(P.logits.view(M, K), target, H * W, out=P.dlogits.view(M, K))

        # ---- backward
        ops.conv_wgrad(P.head[1], P.y, P.dlogits, tuple(self.head[1].weight.shape), dw=self.g_head[1][0], dbias=self.g_head[1][1])
        ops.conv_dgrad(P.head[1], P.dlogits, pk_head[1][1], out=P.dy, relu_x=P.y)              # through the fused ReLU
        ops.conv_wgrad(P.head[0], x_h, P.dy, tuple(self.head[0].weight.shape), dw=self.g_head[0][0], dbias=self.g_head[0][1])
        cur = 0
        d_xh = ops.conv_dgrad(P.head[0], P.dy, pk_head[0][1], out=P.d_xh[cur])
        d_xv = None                                    # the last layer's out_v feeds nothing
        for l in range(L - 1, -1, -1):
            layer, A = model.layers[l], P.act[l]
            x_v, x_h = inputs[l]
            wgrad(l, "horiz_resid", A["out"], d_xh)
            dgrad(l, "horiz_resid", d_xh, P.d_out)
            ops.gated_activation_sum_backward(A["v2h"], A["h_horiz"], A["cond"], P.d_out, out=P.dx_sum, dcond=P.dcond[:B])
            wgrad(l, "horiz_stack", x_h, P.dx_sum)
            wgrad(l, "vert_to_horiz", A["h_vert"], P.dx_sum)
            if d_xv is not None:
                ops.gated_activation_backward_colsum(A["h_vert"], A["cond"], d_xv, out=P.dx_v, dcond=P.dcond[B:])
                dgrad(l, "vert_to_horiz", P.dx_sum, P.d_hvert, add=P.dx_v)
                ops.index_add_rows(label2, P.dcond, n_classes, impl="f32", out=self.g_cls[l])
            else:
                dgrad(l, "vert_to_horiz", P.dx_sum, P.d_hvert)
                ops.index_add_rows(label, P.dcond[:B], n_classes, impl="f32", out=self.g_cls[l])
            wgrad(l, "vert_stack", x_v, P.d_hvert)
            d_xv = dgrad(l, "vert_stack", P.d_hvert, P.d_xv)
            if l > 0:
                d_xh = dgrad(l, "horiz_stack", P.dx_sum, P.d_xh[1 - cur], add=d_xh if layer.residual else None)
            else:                                      # layer 0: both stacks read e
                d_xh = dgrad(l, "horiz_stack", P.dx_sum, P.d_xh[1 - cur], add=d_xv)
            cur = 1 - cur
        ops.index_add_rows(codes.reshape(-1), d_xh.view(M, dim), K, impl="f32", out=self.g_emb)
        return loss[0]

    @torch.no_grad()
    def step(self, codes, label, lengths=None, *, check: bool = True):
        """forward_backward, then one FlatAdam step -> the loss (device scalar) of the parameters BEFORE the step."""
        loss = self.forward_backward(codes, label, lengths, check=check)
        self.opt.step()
        return loss


def prior_labels(prior: GatedPixelCNN, g, B: int):
    """The class labels of a loader batch: the speaker ids g (B,) when the data root has speakers, else zeros.  Validated where
    they are (ValueError for an id outside the prior's classes): free of synchronisation for a loader's host tensors."""
    if g is None:
        return torch.zeros(B, dtype=torch.int64)
    n_classes = prior.layers[0].class_cond_embedding.num_embeddings
    if tuple(g.shape) != (B,) or g.dtype != torch.int64:
        raise ValueError(f"speaker ids must be an int64 tensor of shape ({B},)")
    if int(g.min()) < 0 or int(g.max()) >= n_classes:
        raise ValueError(f"speaker ids outside the prior's [0, {n_classes}) classes")
    return g


def drop_labels(label, p, null_label, generator):
    """Label dropout for classifier-free guidance: label int64 (B,) with label[b] replaced by null_label where a uniform draw
    from the CPU `generator` is < p.  The B draws are made on the host in clip order (one torch.rand(B) call); the replacement
    is a torch.where on the label's own device.  p == 0 draws nothing and returns `label` itself."""
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:
        raise ValueError("drop_labels: p must be a number in [0, 1]")
    if not isinstance(label, torch.Tensor) or label.dim() != 1 or label.dtype != torch.int64:
        raise ValueError("drop_labels: label must be an int64 tensor (B,)")
    if p == 0:
        return label
    if isinstance(null_label, bool) or not isinstance(null_label, numbers.Integral) or null_label < 0:
        raise ValueError("drop_labels: null_label must be an integer >= 0")
    if not isinstance(generator, torch.Generator) or generator.device.type != "cpu":
        raise ValueError("drop_labels: generator must be a CPU torch.Generator")
    drop = torch.rand(label.shape[0], generator=generator) < p
    return torch.where(drop.to(label.device), torch.full_like(label, int(null_label)), label)


def _label_dropout(args, prior, epoch):
    """train_prior's label dropout from args (label_dropout, null_label, label_dropout_seed), validated: None when off, else
    (p, null_label, the epoch's CPU generator, seeded from (seed, epoch))."""
    p = getattr(args, "label_dropout", 0.0)
    null_label = getattr(args, "null_label", None)
    seed = getattr(args, "label_dropout_seed", 0)
    n_classes = prior.layers[0].class_cond_embedding.num_embeddings
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:
        raise ValueError("train_prior: label_dropout must be a number in [0, 1]")
    if null_label is not None and (isinstance(null_label, bool) or not isinstance(null_label, numbers.Integral) or not 0 <= null_label < n_classes):
        raise ValueError(f"train_prior: null_label must be an integer in [0, {n_classes})")
    if p == 0:
        return None
    if null_label is None:
        raise ValueError("train_prior: label_dropout > 0 needs a null_label")
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or isinstance(epoch, bool) or not isinstance(epoch, numbers.Integral):
        raise ValueError("train_prior: label_dropout_seed and epoch must be integers")
    # one stream per (seed, epoch): the pair packed into the generator's 64-bit seed, 32 bits each
    generator = torch.Generator().manual_seed(((int(seed) & 0xFFFFFFFF) << 32) | (int(epoch) & 0xFFFFFFFF))
    return float(p), int(null_label), generator


def train_prior(args, vqvae, prior, step_or_optimizer, train_loader, device, epoch):
    """One epoch of the prior on the codes of the (frozen, never updated) VQ-VAE.  `train_loader` yields
    (x, y, c, g, input_lengths) with c (B, 80, T) mel frames, T a multiple of 4.  step_or_optimizer: a PriorTrainStep (the fused
    step) or a torch optimiser over prior.parameters() (the autograd path: parity / fallback form).  The padded columns of each
    clip are left out of the loss.  Returns the mean of the batches' losses.
    Label dropout (training for classifier-free guidance, GatedPixelCNN.sample(guidance=)): with args.label_dropout = p > 0 each
    clip's label is replaced by args.null_label with probability p before the step (drop_labels), from one CPU generator per
    epoch seeded from (args.label_dropout_seed, epoch).  The three attributes are optional; without them, or with p == 0, the
    epoch is the one without dropout, bit for bit.  A p outside [0, 1], a null_label outside the prior's classes and dropout
    without a null label are a ValueError before the first batch."""
    from .evaluate import codes_from_mels
    fused = isinstance(step_or_optimizer, PriorTrainStep)
    dropout = _label_dropout(args, prior, epoch)
    prior.train()
    total = torch.zeros((), dtype=torch.float64, device=device)
    n_batches = 0
    for batch_idx, (x, y, c, g, input_lengths) in enumerate(train_loader):
        c = c.to(device).unsqueeze(1)
        codes, lengths = codes_from_mels(vqvae, c, input_lengths)
        label = prior_labels(prior, g, len(c)).to(device)
        if dropout is not None:
            label = drop_labels(label, *dropout)
        lengths = lengths.to(device)                    # (validated on the host by codes_from_mels: clipped to [0, W])
        if fused:
            loss = step_or_optimizer.step(codes, label, lengths, check=False)
        else:
            step_or_optimizer.zero_grad()
            loss = prior.loss(codes, label, lengths)
            loss.backward()
            step_or_optimizer.step()
            loss = loss.detach()
        total += loss
        n_batches += 1
        if batch_idx % args.log_interval == 0:
            print('Train Epoch: {} [{}/{}]\tPrior loss: {:.6f}'.format(epoch, batch_idx * len(c), len(train_loader.dataset), loss.item()))
    if n_batches == 0:
        raise ValueError("train_prior: empty loader")
    return float(total / n_batches)
