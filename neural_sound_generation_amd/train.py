"""The reference's per-batch training step (src/train.py:104-148, ljspeech branch) on the HIP path.

Two ways to run it:

  * `train_vqvae(args, model, optimizer, train_loader, device, epoch)` -- same signature and
    behaviour as the reference's function: autograd through the model's fused stacks, three
    F.mse_loss terms, optimizer.step().  Any torch optimizer works (FlatAdam is the fused one).

  * `FusedTrainStep` -- the same arithmetic with no autograd in the loop: forward, the three loss
    terms and their gradients from two fused kernels, explicit backward writing straight into the
    flat gradient bucket, one all-reduce when data-parallel, one Adam kernel.  This is what bench.py
    times.  The zero-pad-to-input-width of train.py:118-120 is folded into the loss kernel (the
    reference bounces through host memory there).
"""
from __future__ import annotations

import os

import numpy as np

import torch
import torch.nn.functional as F

from . import distributed as nsg_dist
from . import engine, functional as Fn, ops
from .optim import FlatAdam


# The bf16 step without an fp32 z_q (see _forward_backward); NSG_LEAN_VQ=0 keeps the materialised form.
LEAN_VQ = os.environ.get("NSG_LEAN_VQ", "1") == "1"
# ... and without an fp32 z_e either: the encoder's closing BatchNorm + skip pass is not run, its three consumers (search, loss /
# encoder gradient, per-code sums) form z_e from its bf16 sources while they load it -- the same bits, 0.84 GB less traffic per
# step at the bench's shape.  NSG_ZE_FROM_SOURCES=0 keeps the materialised form.
ZE_FROM_SOURCES = os.environ.get("NSG_ZE_FROM_SOURCES", "1") == "1"


def comm_split(opt: FlatAdam, front, back) -> int:
    """Where a data-parallel step may cut opt's communication buffer in two, in floats from its start: `back` (gradient views that
    are final early: decoder, speaker table) is then all-reduced while `front` (encoder, codebook) is still being written.  The
    split is the lowest start of a back view, so no back view lies in front of it; it stands only if every front view ends at or
    before it, and is 0 -- one collective at the end -- otherwise.  (A tail reserved with opt.reserve_tail lies behind opt.total,
    so behind any split.)"""
    lo = opt.flat_grad.data_ptr()
    split = min((t.data_ptr() - lo) // 4 for t in back)
    if 0 < split < opt.total and all((t.data_ptr() - lo) // 4 + t.numel() <= split for t in front):
        return split
    return 0


class FusedTrainStep:
    def __init__(self, model, lr: float = 1e-3, beta: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group=None, optimizer: FlatAdam | None = None, revive_every: int = 0, revive_min_count: int = 1,
                 revive_seed: int = 0, codebook_init: str | None = None):
        """revive_every = R > 0 (extension, off by default): every step ends with the codebook usage kernel on its indices, every
        R-th step re-seeds the codes used fewer than revive_min_count times since the last revival from that step's z_e
        (codebook.CodebookReviver; revive_seed seeds its row choice).  codebook_init = "data": the first step ends by
        initialising the whole codebook from its z_e.  With both off the step launches and holds nothing new."""
        self.model = model
        self.beta = float(beta)
        self.group = process_group
        self.opt = optimizer if optimizer is not None else FlatAdam(model.parameters(), lr=lr, betas=betas, eps=eps)
        self.world = nsg_dist.world_size(process_group)
        self.dtype = getattr(model, "compute_dtype", torch.float32)
        self.ema = getattr(model.codebook, "ema_decay", None) is not None
        if self.world > 1:
            # every replica starts from rank 0's state: the parameter bucket, and -- packed into one flat tensor, one more
            # broadcast -- everything outside it: BatchNorm running statistics and counters, an EMA-trained codebook
            # (requires_grad=False keeps it out of the bucket) with its ema_count / ema_sum buffers
            nsg_dist.broadcast_flat(self.opt.flat_param, 0, process_group)
            if getattr(self.opt, "shadow", None) is not None:      # the averaged weights (weight_ema_decay) follow rank 0's too
                nsg_dist.broadcast_flat(self.opt.shadow, 0, process_group)
            nsg_dist.broadcast_tensors_packed(nsg_dist.state_outside(model, self.opt), 0, process_group)
        if self.ema:
            # [n (K, padded to 256 bytes) | sum z (K x D)] lives BEHIND the gradients: ONE all-reduce carries both
            K, D = model.codebook.embedding.weight.shape
            self._n_pad = (K + 63) // 64 * 64
            tail = self.opt.reserve_tail(self._n_pad + K * D)
            self.ema_n = tail[:K]
            self.ema_s = tail[self._n_pad:].view(K, D)
        # the codebook scatter-add as a sorted segment sum (fp32, deterministic; NSG_SCATTER_IMPL=onehot restores the one-hot
        # GEMMs: bf16x2 on the bf16 pipe in the bf16 mode, exact fp32 products in the fp32 mode)
        if os.environ.get("NSG_SCATTER_IMPL", "sorted") == "sorted":
            self.scatter_impl = "sorted"
        else:
            self.scatter_impl = "bf16x2" if self.dtype == torch.bfloat16 else "f32"
        self.encP = engine.encoder_params(model.encoder)
        self.decP = engine.decoder_params(model.decoder)
        self.codebook = model.codebook.embedding.weight
        g_enc = self.opt.grads_for(engine.encoder_param_list(self.encP))
        g_dec = self.opt.grads_for(engine.decoder_param_list(self.decP))
        self.g_enc, self.g_dec = engine.encoder_grads(g_enc), engine.decoder_grads(g_dec)
        self.g_code = None if self.ema else self.opt.grads_for([self.codebook])[0]
        self.spk = getattr(model, "speaker_embedding", None)
        self.g_spk = self.opt.grads_for([self.spk.weight])[0] if self.spk is not None else None
        # the F0 table of an F0-conditioned decoder (VQVAE(n_f0_bins=)): registered after the speaker table, so its slot lies behind it
        self.f0 = getattr(model, "f0_embedding", None)
        self.g_f0 = self.opt.grads_for([self.f0.weight])[0] if self.f0 is not None else None
        # Data parallel: the communication buffer is [encoder | codebook | decoder | speaker table | F0 table | EMA statistics]; everything
        # from the decoder's first gradient on is final when the decoder's backward has been enqueued, BEFORE the encoder's
        # backward starts, so that part is all-reduced on the collective's own stream beside the encoder backward and only the
        # front part waits for the end of the step (two collectives, the first one hidden).
        # (An optimiser with another parameter order: comm_split is 0, one collective at the end.)
        self._comm_split = comm_split(self.opt, front=g_enc + ([] if self.g_code is None else [self.g_code]),
                                      back=g_dec + [t for t in (self.g_spk, self.g_f0) if t is not None])
        self._reduce = None               # nsg_dist.TwoPartAllReduce over the communication buffer (made on first use: reserve_tail may still grow it)
        self._stepping = False            # collectives only from step(): forward_backward() alone never communicates
        # test hook: (N,) int64 code indices to use INSTEAD of the search's (the search still runs and is ignored).  Lets a test
        # compare this mode's backward with another evaluation's on the SAME codes (tests/test_gpu_model.py, bf16 fidelity).
        self.force_indices = None
        self.reviver = None
        if revive_every or codebook_init is not None:
            from .codebook import CodebookReviver
            self.reviver = CodebookReviver(model.codebook, every=revive_every, min_count=revive_min_count, seed=revive_seed,
                                           init=codebook_init, process_group=process_group)
        # z_e of the step in flight (rows, or their sources with the BatchNorm's gamma / beta as they were BEFORE the optimiser
        # step): kept only on a step that ends with a revival -- the host knows before the forward pass -- and in a captured
        # graph, whose replays cannot choose (the graph keeps them alive with its other buffers)
        self._keep_rows = False
        self._kept_rows = None

    @torch.no_grad()
    def forward_backward(self, c: torch.Tensor, g: torch.Tensor | None = None, f0_bins: torch.Tensor | None = None,
                         target: torch.Tensor | None = None):
        """c: (B,1,80,T) float32 on the GPU; g: optional (B,) int64 speaker ids (speaker-conditioned
        decoder extension); f0_bins: optional (B, T // 4) int64 F0 bins in [0, n_f0_bins] on the GPU, one per latent column
        (F0-conditioned decoder extension, audio.f0_bins; the kernel clamps them, nothing here reads them back); target: optional
        (B,1,80,T) float32 on c's device, what the reconstruction loss compares the decoder's output against in place of c (the
        encoder still sees c: a perturbed input with the clean mel as the target, audio.perturb_pitch).  It takes c's place as the
        output layer's mse_target: no launch is added, and None is the step as it was, bit for bit.  Fills the flat
        gradient bucket; returns the three loss tensors (device scalars; nothing here synchronises with the host)."""
        model = self.model
        if not model.training:
            raise RuntimeError("FusedTrainStep needs model.train()")
        x = Fn.to_nhwc(c)
        B, H, T, _ = x.shape
        if f0_bins is not None:
            if self.f0 is None:
                raise ValueError("FusedTrainStep: f0_bins given to a model without an F0 table (VQVAE(..., n_f0_bins=N))")
            if not isinstance(f0_bins, torch.Tensor) or tuple(f0_bins.shape) != (B, T // 4) or f0_bins.dtype != torch.int64 or f0_bins.device != x.device:
                raise ValueError(f"FusedTrainStep: f0_bins must be an int64 tensor of shape ({B}, {T // 4}) on the batch's device")
            f0_bins = f0_bins.contiguous()
        if target is not None:
            if (not isinstance(target, torch.Tensor) or target.shape != c.shape or target.dtype != torch.float32 or target.device != c.device):
                raise ValueError(f"FusedTrainStep: target must be a float32 tensor of c's shape {tuple(c.shape)} on the batch's device")
            target = Fn.to_nhwc(target)
        with engine.deferred_batch_counters():
            return self._forward_backward(x, g, B, H, T, f0_bins, target)

    def _forward_backward(self, x, g, B, H, T, bins=None, target=None):
        tgt = x if target is None else target          # what the reconstruction loss compares against
        enc_packs, dec_packs = engine.pack_all(self.encP, self.decP, B, H, T, self.dtype)
        K, D = self.codebook.shape
        search = getattr(self.model.codebook, "search_impl", "mfma")
        # bf16 mode: z_q is never materialised in fp32 -- the search writes the decoder's (ReLU'd, bf16) input itself, with the
        # clip's speaker row added when the decoder is speaker-conditioned; the losses read codebook[idx], the codebook gradient
        # comes from per-code sums of z_e
        lean = LEAN_VQ and search == "bf16x3" and self.dtype == torch.bfloat16 and D % 8 == 0
        # ... and z_e itself only as its sources, where all of its consumers take them (the encoder may still decline: ze is then a tensor)
        defer = (lean and ZE_FROM_SOURCES and self.force_indices is None and self.scatter_impl == "sorted" and ops.bnres_rows_supported(D)
                 and ops.index_add_sorted_supported(x.numel(), D, K) and ops.vq_losses_indexed_bn_supported(D))
        ze, es = engine.encoder_forward(x, self.encP, True, dtype=self.dtype, packs=enc_packs, defer_closing_bn=defer)
        # the encoder's closing BatchNorm as rows given by their sources (ops.BnResRows), or None where the block ran the separate
        # operators: z_e itself where the forward deferred it, and -- deferred or not -- what the loss pass needs for bn= further
        # down (fetched once, here: these are views, nothing is launched)
        bn2 = engine.encoder_closing_bn(es, self.encP) if lean else None
        ze_rows = bn2 if ze is None else ze.view(-1, D)
        ze_shape = es.ze_shape
        ze_numel = ze_rows.shape[0] * D
        if self._keep_rows:
            self._kept_rows = ze_rows._replace(gamma=ze_rows.gamma.clone(), beta=ze_rows.beta.clone()) if ze is None else ze_rows
        spk_rows = None
        if self.spk is not None and g is not None:
            g = g.view(-1).to(torch.int64).contiguous()
            spk_rows = ops.gather_rows(self.spk.weight.detach(), g)          # (B, D) fp32
        if self.force_indices is not None:
            idx = self.force_indices.view(-1).to(device=ze.device, dtype=torch.int64).contiguous()     # (ze is a tensor here: defer is off)
            if idx.numel() != ze.numel() // D:
                raise ValueError("force_indices must hold one code index per latent row")
            zq = ops.gather_rows(self.codebook.detach(), idx).view_as(ze)
            zdec = zq
            if lean and bins is not None:
                zdec, zq = ops.add_cond(zq, self.f0.weight.detach(), bins, clip_rows=spk_rows, relu=True, out_dtype=self.dtype), None
            elif lean:
                zdec = ops.add_per_clip(zq, spk_rows) if spk_rows is not None else zq
                zdec, zq = ops.convert(zdec, self.dtype, relu=True), None
        elif lean and bins is not None:
            # the search writes the indices alone; the decoder's input is gathered through them with both conditioning rows added
            idx, _, _ = ops.vq_forward(ze_rows, self.codebook.detach(), want_codes=False, impl=search)
            zq = None
            zdec = ops.add_cond(self.codebook.detach(), self.f0.weight.detach(), bins, idx=idx, clip_rows=spk_rows, relu=True,
                                out_dtype=self.dtype, grid=tuple(ze_shape[:3]))
        elif lean:
            idx, _, _, zdec = ops.vq_forward(ze_rows, self.codebook.detach(), want_codes=False, impl=search, codes_bf16="relu",
                                             clip_rows=spk_rows)
            zq = None
            zdec = zdec.view(ze_shape)
        else:
            idx, zq, _ = ops.vq_forward(ze.view(-1, D), self.codebook.detach(), want_codes=True, impl=search)
            zq = zq.view_as(ze)
            zdec = zq
        if bins is not None and not lean:
            zdec = ops.add_cond(zq, self.f0.weight.detach(), bins, clip_rows=spk_rows, out_dtype=self.dtype)
        elif spk_rows is not None and not lean:
            zdec = ops.add_per_clip(zq, spk_rows, out_dtype=self.dtype)
        # loss_recons = mse(zero-pad(x_tilde), c) and d/dx_tilde             (train.py:118-129)
        xt, ds = engine.decoder_forward(zdec, self.decP, True, dtype=self.dtype, packs=dec_packs, zq_is_relu=lean, mse_target=tgt,
                                        mse_dbias=self.g_dec.convt6.bias)
        if isinstance(xt, engine.FusedLoss):    # the fused output layer formed the loss and the gradient at the Tanh's input with the image
            loss_recons = xt.loss
            dzq, _ = engine.decoder_backward(xt.dpre, ds, self.decP, need_dz=True, dxt_is_pre_tanh=True, gout=self.g_dec)
        else:
            loss_recons, dxt = ops.mse_padded(xt, tgt, B * H, xt.shape[2], T)
            dzq, _ = engine.decoder_backward(dxt, ds, self.decP, need_dz=True, gout=self.g_dec)
        colsum = None
        if self.f0 is not None:
            if bins is not None:    # d loss / d F0 rows = per-column sums of dzq over the latent rows, scattered to the bins
                colsum = ops.column_sum(dzq.view(ze_shape))                 # (B, W, D) fp32: dzq is read once for both tables
                gf = ops.index_add_rows(bins.view(-1), colsum.view(-1, D), self.f0.weight.shape[0])
                ops.add(gf, None, out=self.g_f0)
            else:
                self.g_f0.zero_()
        if self.spk is not None:
            if g is not None:   # d loss / d speaker rows = per-clip pixel sums of dzq, scattered to the speakers
                gs = ops.index_add_rows(g, ops.clip_colsum(dzq if colsum is None else colsum, B), self.spk.weight.shape[0])
                ops.add(gs, None, out=self.g_spk)
            else:
                self.g_spk.zero_()
        if self.ema:    # per-code counts and sums of the assigned encoder rows straight into the communication buffer's tail
            ops.index_add_rows(idx, ze_rows, K, impl=self.scatter_impl, out=self.ema_s, counts=self.ema_n)
        self._reduce_back_part()        # decoder, speaker table, EMA statistics: final from here on (no-op on one rank / in a graph)
        # loss_vq = mse(z_q, sg(z_e)) -> codebook; loss_commit = mse(z_e, sg(z_q)) -> encoder,
        # plus the straight-through gradient from the decoder               (train.py:131-134)
        bn2_sums = None
        if lean:
            # dz is the incoming gradient of the encoder's closing BatchNorm: its backward sums are formed while dz is written
            if bn2 is not None and bn2.h.dtype == self.dtype and ops.vq_losses_indexed_bn_supported(D):
                loss_vq, dz, dg, db = ops.vq_losses_indexed(ze_rows, self.codebook.detach(), idx, dz_scale=self.beta, dz_add=dzq.view(-1, D),
                                                            grad_dtype=self.dtype, bn=(bn2.h, bn2.mean, bn2.invstd),
                                                            dgamma=self.g_enc.res5.bn2.weight, dbeta=self.g_enc.res5.bn2.bias)
                bn2_sums = (dg, db)
            else:
                loss_vq, dz = ops.vq_losses_indexed(ze_rows, self.codebook.detach(), idx, dz_scale=self.beta, dz_add=dzq.view(-1, D),
                                                    grad_dtype=self.dtype)
            dz = dz.view(ze_shape)
            if not self.ema:    # d loss_vq / d e_k = 2/numel * sum over the rows assigned to k of (e_k - z) = 2/numel * (n_k e_k - s_k)
                s, n = ops.index_add_rows(idx, ze_rows, K, want_counts=True, impl=self.scatter_impl)
                ops.codebook_grad_from_sums(self.codebook.detach(), n, s, 2.0 / ze_numel, out=self.g_code)
        elif self.ema:
            # EMA codebook (extension): no codebook gradient; per-code counts and sums of the assigned
            # encoder rows are the statistics every rank contributes (summed over ranks in step())
            loss_vq, dz, _ = ops.vq_losses(ze, zq, dz_scale=self.beta, dq_scale=1.0, dz_add=dzq, want_dq=False, grad_dtype=self.dtype)
        else:
            loss_vq, dz, dq = ops.vq_losses(ze, zq, dz_scale=self.beta, dq_scale=1.0, dz_add=dzq, grad_dtype=self.dtype)
            self._codebook_grad(idx, dq.view(-1, D), K)
        engine.encoder_backward(dz, es, self.encP, gout=self.g_enc, bn2_sums=bn2_sums)
        self.last_indices = idx
        return loss_recons, loss_vq, loss_vq

    def _reduce_back_part(self):
        """Start the all-reduce of [decoder | speaker | EMA statistics] (called when they are final: the collective waits for the
        kernels enqueued so far, then runs on its own stream beside the encoder backward).  step() joins it before Adam."""
        if self.world > 1 and self._comm_split > 0 and self._stepping and not torch.cuda.is_current_stream_capturing():
            self._two_part().start_back()

    def _two_part(self):
        if self._reduce is None or self._reduce.flat.data_ptr() != self.opt.flat_comm.data_ptr() or self._reduce.flat.numel() != self.opt.flat_comm.numel():
            self._reduce = nsg_dist.TwoPartAllReduce(self.opt.flat_comm, self._comm_split, self.group)
        return self._reduce

    def _codebook_grad(self, idx, dq, K):
        g = ops.index_add_rows(idx, dq, K, impl=self.scatter_impl)
        ops.add(g, None, out=self.g_code)

    # ---- HIP graph of forward + backward (optional) ------------------------------------------------------------
    # The ~140 kernel launches that fill the gradient bucket are captured once and replayed (hipGraph through
    # torch.cuda.CUDAGraph: every ctypes launch goes to torch's current stream, which is the capturing stream).  The
    # optimiser step stays outside (its bias-correction scalars change every step), as do the collectives.
    @torch.no_grad()
    def capture(self, c: torch.Tensor, g: torch.Tensor | None = None, warmup: int = 2, f0_bins: torch.Tensor | None = None,
                target: torch.Tensor | None = None):
        """Capture forward_backward for inputs of c's shape.  The warm-up steps are REAL training steps.  g, f0_bins and target are
        kept in static buffers every replay refills; a graph captured with (without) any of them is replayed only for a step that
        gives (omits) it too -- any other step runs eagerly.  So a graph captured without a target is never replayed for a step
        that has one: its launches carry c's buffer as the loss target."""
        # The captured launches carry the scratch buffer's ADDRESS, and ops.WS keeps one buffer per (device, stream).  So the
        # warm-up steps (first-use work: LDS attributes, workspace growth -- and they are REAL training steps) run on the very
        # stream the capture then uses: the capture finds the warmed-up buffer under its own key and must not outgrow it.  A
        # later call on that stream that needs more scratch makes the workspace allocate a new buffer and drop the old one; this
        # graph holds a reference to the old one (_graph_ws), so its replays never touch memory someone else owns.
        self._graph_stream = torch.cuda.Stream(device=c.device)
        self._graph_stream.wait_stream(torch.cuda.current_stream(c.device))
        with torch.cuda.stream(self._graph_stream):
            for _ in range(warmup):
                self.step(c, g, f0_bins, target)
            self._static_c = c.clone()
            self._static_g = g.clone() if g is not None else None
            self._static_bins = f0_bins.clone() if f0_bins is not None else None
            self._static_target = target.clone() if target is not None else None
            ws = ops.WS.current(c.device)              # (this stream's buffer)
        torch.cuda.current_stream(c.device).wait_stream(self._graph_stream)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        self._keep_rows = self.reviver is not None
        try:
            with torch.cuda.graph(self._graph, stream=self._graph_stream):
                self._graph_losses = self.forward_backward(self._static_c, self._static_g, self._static_bins, self._static_target)
                ws_after = ops.WS.current(c.device)
        finally:
            self._keep_rows = False
        self._graph_rows, self._kept_rows = self._kept_rows, None     # every replay refills them
        if ws is None or ws_after is not ws:
            self._graph = None
            raise RuntimeError("FusedTrainStep.capture: the workspace grew during capture (warm-up steps must see the captured shapes)")
        self._graph_ws = ws
        return self

    def _replay(self, c, g, f0_bins=None, target=None):
        self._static_c.copy_(c)
        if g is not None:
            self._static_g.copy_(g)
        if f0_bins is not None:
            self._static_bins.copy_(f0_bins)
        if target is not None:
            self._static_target.copy_(target)
        self._graph.replay()
        return self._graph_losses

    @torch.no_grad()
    def step(self, c: torch.Tensor, g: torch.Tensor | None = None, f0_bins: torch.Tensor | None = None, target: torch.Tensor | None = None):
        revive = self.reviver is not None and self.reviver.next_step_revives()
        if (getattr(self, "_graph", None) is not None and c.shape == self._static_c.shape and (g is None) == (self._static_g is None)
                and (f0_bins is None) == (self._static_bins is None)
                and (f0_bins is None or (f0_bins.shape == self._static_bins.shape and f0_bins.dtype == torch.int64))
                and (target is None) == (getattr(self, "_static_target", None) is None)
                and (target is None or (target.shape == self._static_target.shape and target.dtype == torch.float32))):
            losses = self._replay(c, g, f0_bins, target)
            rows = self._graph_rows if revive else None
        else:
            self._stepping, self._keep_rows = True, revive
            try:
                losses = self.forward_backward(c, g, f0_bins, target)
            finally:
                self._stepping = self._keep_rows = False
            rows, self._kept_rows = self._kept_rows, None
        if self.world > 1:
            # the gradient bucket and behind it (EMA mode) the per-code counts and sums: the back part is already in flight
            # (_reduce_back_part), the front part (encoder, codebook) goes now; a replayed graph holds no collective: one for all
            self._two_part().finish()
        self.opt.step(grad_scale=1.0 / self.world)
        if self.ema:
            self.apply_ema()
        if self.reviver is not None:
            # outside the captured graph, like Adam and the collectives; data parallel: the gradients' all-reduce is joined above
            self.reviver.end_step(self.last_indices, rows, self.opt)
        return losses

    def codebook_stats(self) -> dict:
        """CodebookReviver.stats() of this step's reviver: perplexity and codes in use of the last batch, codes revived by the last
        revival and in total.  Synchronises with the device."""
        if self.reviver is None:
            raise RuntimeError("FusedTrainStep.codebook_stats: built without revive_every / codebook_init")
        return self.reviver.stats()

    @torch.no_grad()
    def apply_ema(self, n: torch.Tensor | None = None, s: torch.Tensor | None = None):
        """n (K,), s (K, D): per-code counts and sums of the encoder rows, summed over ranks (default: this step's, as
        left in the communication buffer by the all-reduce): the identical update on every rank."""
        cb = self.model.codebook
        ops.vq_ema_update(self.codebook.data, cb.ema_count, cb.ema_sum, self.ema_n if n is None else n.contiguous(),
                          self.ema_s if s is None else s.contiguous(), decay=cb.ema_decay, eps=cb.ema_eps)


def vqvae_loss_terms(c, x_tilde, z_e_x, z_q_x):
    """train.py:118-133 on device tensors (autograd path): zero-pad without the host round trip."""
    if x_tilde.size(3) != c.size(3):
        target = F.pad(x_tilde, (0, c.size(3) - x_tilde.size(3)))
    else:
        target = x_tilde
    loss_recons = F.mse_loss(target, c)
    loss_vq = F.mse_loss(z_q_x, z_e_x.detach())
    loss_commit = F.mse_loss(z_e_x, z_q_x.detach())
    return loss_recons, loss_vq, loss_commit


def train_vqvae(args, model, optimizer, train_loader, device, epoch):
    """Drop-in for the reference's train_vqvae (src/train.py:104-148, ljspeech branch).
    `train_loader` yields (x, y, c, g, input_lengths) with c: (B, 80, T) mel frames."""
    model.train()
    train_loss = 0
    n_batches = 0
    for batch_idx, (x, y, c, g, input_lengths) in enumerate(train_loader):
        optimizer.zero_grad()
        c = c.to(device).unsqueeze(1)
        x_tilde, z_e_x, z_q_x = model(c)
        loss_recons, loss_vq, loss_commit = vqvae_loss_terms(c, x_tilde, z_e_x, z_q_x)
        loss = loss_recons + loss_vq + args.beta * loss_commit
        loss.backward()
        optimizer.step()
        train_loss = loss_recons.item() + loss_vq.item()
        n_batches += 1
        if batch_idx % args.log_interval == 0:
            print('Train Epoch: {} [{}/{}]\tLoss: {:.6f}'.format(epoch, batch_idx * len(c), len(train_loader.dataset), train_loss))
    return train_loss


def train_conditioned(args, model, step, train_loader, device, epoch, tracker="yin", tracker_options=None, pitch_perturb=None, generator=None):
    """One epoch of a speaker- and / or F0-conditioned VQ-VAE on the fused step (an extension: train_vqvae above stays the
    reference's, which ignores g).  `train_loader` yields (x, y, c, g, input_lengths) as for train_vqvae, or the six-tuple
    (x, y, c, g, input_lengths, f0_bins) of a resident loader with an F0 track (data.ResidentMelLoader(f0=)); `step` is the model's
    FusedTrainStep.  Per batch: g goes to the device; for a model with an F0 table (VQVAE(n_f0_bins=)) a sixth element is the bins
    and goes straight to the step (moved to the device if it is not there; x is not needed and the tracker arguments are unused);
    otherwise the F0 of the batch's audio x (B, 1, T * 256) is tracked on the device (tracker, tracker_options: evaluate.test_conversion_f0's; lengths = input_lengths;
    F0 frame t is mel frame t), its first 4 * (T // 4) frames become the bins of the T // 4 latent columns (audio.f0_bins over the
    model's n_f0_bins and f0_range, each clip's input_lengths // 256 frames valid) and step.step(c, g, f0_bins=bins) runs.
    (The two sources differ at a crop's edge frames: data.ResidentMelCorpus.track_f0.)
    Returns the last batch's loss_recons + loss_vq, as train_vqvae does.  ValueError before anything is launched: a tracker or
    options that do not exist; a model with an F0 table and a batch with neither bins nor audio (get_data_loaders(with_audio=True)).
    pitch_perturb=(low, high) in semitones (None, the default: the loop as it was): information perturbation.  The bins still
    come from the batch as given; then the encoder's input is replaced by c' = the first T frames of audio.melspectrogram of
    audio.perturb_pitch(x, input_lengths, generator, pitch_perturb, tracker, tracker_options) -- each clip's pitch moved by a
    random shift with its formants and length kept -- while the loss target stays c: step.step(c', g, f0_bins=bins, target=c).
    The codes then no longer tell the pitch of the mel to be reproduced, and an F0-conditioned decoder has to take it from the
    bins.  generator: the CPU torch.Generator of the shifts (None: a new one seeded with `epoch`).  It needs the batch's audio:
    a batch without x (a resident loader built without audio=True; a host loader built without with_audio=True) is a ValueError
    before anything of that batch is launched, as are a range outside [-12, 12] and a generator that is not a CPU one."""
    from . import audio
    from .evaluate import _f0_tracker, batch_conditioning
    track = _f0_tracker("train_conditioned", tracker, tracker_options)
    if pitch_perturb is not None:
        lo, hi = audio._range("train_conditioned", "pitch_perturb", pitch_perturb)
        if lo < -12.0 or hi > 12.0:
            raise ValueError(f"train_conditioned: pitch_perturb {pitch_perturb!r} outside [-12, 12] semitones")
        if generator is None:
            generator = torch.Generator().manual_seed(int(epoch))
        elif not isinstance(generator, torch.Generator) or generator.device.type != "cpu":
            raise ValueError("train_conditioned: generator must be a CPU torch.Generator")
    model.train()
    train_loss, last = 0, None
    for batch_idx, batch in enumerate(train_loader):
        if pitch_perturb is not None and batch[0] is None:
            raise ValueError("train_conditioned: pitch_perturb needs the batch's audio and the loader yields none: "
                             "get_data_loaders(with_audio=True) or get_resident_loaders(audio=True) (a resident loader without "
                             "audio=True keeps no audio)")
        c, g_d, bins = batch_conditioning("train_conditioned", model, batch, device, track)
        if pitch_perturb is not None:
            T = c.shape[3]
            lens = np.asarray(batch[4].cpu() if torch.is_tensor(batch[4]) else batch[4]).astype(np.int64)
            wav = batch[0].view(batch[0].shape[0], -1).to(device).contiguous()
            moved, _ = audio.perturb_pitch(wav, lens, generator, (lo, hi), tracker, tracker_options)
            mel = audio.melspectrogram(moved, lengths=lens)
            if mel.shape[2] < T:
                raise ValueError(f"train_conditioned: the batch's audio gives {mel.shape[2]} mel frames, its mel has {T}")
            c_in = mel[:, None, :, :T].contiguous()
            loss_recons, loss_vq, _ = step.step(c_in, g_d, f0_bins=bins, target=c)
        else:
            loss_recons, loss_vq, _ = step.step(c, g_d, f0_bins=bins) if bins is not None else step.step(c, g_d)
        last = loss_recons + loss_vq
        if batch_idx % args.log_interval == 0:      # (the only read-back: the fused step itself never waits for the device)
            print('Train Epoch: {} [{}/{}]\tLoss: {:.6f}'.format(epoch, batch_idx * len(c), len(train_loader.dataset), float(last)))
    return float(last) if last is not None else train_loss
