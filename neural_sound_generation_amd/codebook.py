"""Codebook usage statistics and dead-code revival for VQ-VAE training (extension; the reference has neither).

The reference's plain nearest-neighbour codebook, initialised U(-1/K, 1/K), ends up with a handful of live codes (DESIGN.md
"Codebook usage and revival": perplexity 3.5 of 512).  `CodebookReviver` is the opt-in remedy most VQ-VAE trainers ship:

  * every step, `observe(indices, z_e)` histograms the step's code indices on the device (ops.code_usage) into a running
    window and leaves the batch's perplexity and number of codes in use in a device buffer;
  * every R-th step, `revive(optimizer)` re-seeds the codes the window saw fewer than `min_count` times from rows of the current
    encoder output (ops.vq_revive): the j-th dead code, in index order, takes row (base_row + j * stride) mod N, base_row drawn
    from a seeded random.Random, stride a fixed prime.  The optimiser's moments of those rows are cleared, an EMA codebook's
    ema_count / ema_sum re-seeded; live rows are not touched; the window starts again from zero;
  * `revive(revive_all=True)` initialises the whole codebook from the batch.

With the options off nothing here runs: FusedTrainStep's defaults construct no reviver.

State (window, counters, the random generator) lives in this object, NOT in VQEmbedding buffers: the model's state_dict keys
stay the reference's, so checkpoints keep moving both ways.  A run resumed from a checkpoint simply starts with an empty window
(the first revival after a resume sees only the steps since) and a generator back at its seed.
"""
from __future__ import annotations

import random

import torch

from . import distributed as nsg_dist
from . import functional as Fn, ops

# The stride between the rows taken by successive dead codes: a prime, so it is coprime to every N it does not divide -- the
# chosen rows are then pairwise distinct while there are at most N dead codes (beyond that rows repeat).
STRIDE = 1_000_003
STRIDE_ALT = 1_000_033      # (also prime) when N is a multiple of the first


def revive_stride(N: int) -> int:
    return STRIDE_ALT if N % STRIDE == 0 else STRIDE


class CodebookReviver:
    def __init__(self, codebook, every: int = 0, min_count: int = 1, seed: int = 0, init: str | None = None, process_group=None):
        """codebook: the model's VQEmbedding (its .embedding.weight is the (K, D) codebook; ema_count / ema_sum are used when it
        is EMA-trained).  every = R > 0: end_step() revives on every R-th step; init = "data": the first step ends with
        revive(revive_all=True).  A caller that drives observe() / revive() itself may leave both off."""
        if init not in (None, "data"):
            raise ValueError('CodebookReviver: init must be None or "data"')
        if int(every) < 0 or int(min_count) < 0:
            raise ValueError("CodebookReviver: every and min_count must not be negative")
        self.module = codebook
        self.weight = codebook.embedding.weight
        self.K, self.D = self.weight.shape
        self.every, self.min_count, self.init = int(every), int(min_count), init
        self.group = process_group
        self.rng = random.Random(seed)
        self.steps = 0              # steps observed
        self.events = 0             # revive() calls
        self.rows = None            # the encoder rows of the step in flight (held only between observe() and revive())
        dev = self.weight.device
        self.window = torch.zeros(self.K, dtype=torch.int32, device=dev)
        self.batch_counts = torch.zeros(self.K, dtype=torch.int32, device=dev)
        self.slot = torch.full((self.K,), -1, dtype=torch.int32, device=dev)
        self.usage_stats = torch.zeros(2, dtype=torch.float64, device=dev)      # [perplexity, codes in batch]
        self.revive_stats = torch.zeros(2, dtype=torch.int64, device=dev)       # [revived last, revived total]

    # ---- host policy -----------------------------------------------------------------------------------------------------------
    def next_step_revives(self) -> bool:
        """Will the step about to run end with a revival?  Known before its forward pass: a caller keeps z_e only then."""
        return self._all_next() or (self.every > 0 and (self.steps + 1) % self.every == 0)

    def _all_next(self) -> bool:
        return self.init == "data" and self.steps == 0

    def draw(self, N: int):
        """(base_row in [0, N), stride coprime to N) of the next revival."""
        return self.rng.randrange(N), revive_stride(N)

    # ---- device work -------------------------------------------------------------------------------------------------------------
    def _as_rows(self, z_e):
        if isinstance(z_e, ops.BnResRows):
            return z_e
        z_e = z_e.detach()
        if z_e.dim() == 4:          # the reference's (B, D, H, W): permuted to rows (a copy unless the storage is channels-last)
            if z_e.shape[1] != self.D:
                raise ValueError(f"CodebookReviver: z_e has {z_e.shape[1]} channels, the codebook {self.D}")
            return Fn.to_nhwc(z_e).view(-1, self.D)
        if z_e.dim() != 2 or z_e.shape[1] != self.D:
            raise ValueError(f"CodebookReviver: z_e must be (N, {self.D}) rows, a BnResRows or a (B, {self.D}, H, W) tensor")
        return z_e.contiguous()

    @torch.no_grad()
    def observe(self, indices, z_e=None):
        """indices: the step's code indices (any shape, int64); z_e: the step's encoder output -- (N, D) fp32 rows, an
        ops.BnResRows, or the reference-layout (B, D, H, W) tensor -- needed only when revive() follows."""
        ops.code_usage(indices.detach().reshape(-1).contiguous(), self.K, self.window, stats=self.usage_stats, batch_counts=self.batch_counts)
        self.rows = self._as_rows(z_e) if z_e is not None else None
        self.steps += 1

    @torch.no_grad()
    def revive(self, optimizer=None, revive_all: bool = False):
        """Re-seed the dead codes from the rows given to the last observe().  optimizer: the codebook's optimiser, whose moments of
        the revived rows are cleared (a FlatAdam's in the kernel itself, any other torch optimizer's exp_avg / exp_avg_sq on
        the device through `slot`).  Data parallel: the window is summed over ranks first, every rank then runs the kernel on
        the identical dead set, and rank 0's codebook (and EMA statistics) is broadcast."""
        rows = self.rows
        if rows is None:
            raise RuntimeError("CodebookReviver.revive: no encoder rows (pass z_e to the observe() before it)")
        self.rows = None
        world = nsg_dist.world_size(self.group)
        if world > 1:
            nsg_dist.allreduce_sum_(self.window, self.group)
        base_row, stride = self.draw(rows.shape[0])
        m = v = None
        flat = optimizer is not None and hasattr(optimizer, "exp_avg") and hasattr(optimizer, "offsets")
        if flat:
            for p, off in zip(optimizer._params, optimizer.offsets):
                if p is self.weight:
                    n = self.K * self.D
                    m, v = optimizer.exp_avg[off:off + n].view(self.K, self.D), optimizer.exp_avg_sq[off:off + n].view(self.K, self.D)
        ema = getattr(self.module, "ema_decay", None) is not None
        ops.vq_revive(rows, self.weight.data, self.window, min_count=self.min_count, base_row=base_row, stride=stride, adam_m=m, adam_v=v,
                      ema_count=self.module.ema_count if ema else None, ema_sum=self.module.ema_sum if ema else None, slot=self.slot,
                      stats=self.revive_stats, revive_all=revive_all)
        torch.autograd.graph.increment_version(self.weight)      # written through a raw pointer
        if optimizer is not None and not flat:
            st = optimizer.state.get(self.weight, {})
            dead = (self.slot >= 0).unsqueeze(1)
            for key in ("exp_avg", "exp_avg_sq"):
                if key in st:
                    st[key].masked_fill_(dead, 0)
        if world > 1:
            if ema:
                nsg_dist.broadcast_tensors_packed([self.weight.data, self.module.ema_count, self.module.ema_sum], 0, self.group)
            else:
                nsg_dist.broadcast_flat(self.weight.data, 0, self.group)
        self.events += 1

    def end_step(self, indices, z_e=None, optimizer=None):
        """One training step's share: observe, then revive when this step is due (next_step_revives() said so beforehand)."""
        due, everything = self.next_step_revives(), self._all_next()
        self.observe(indices, z_e if due else None)
        if due:
            self.revive(optimizer, revive_all=everything)

    def stats(self) -> dict:
        """The last observed batch's perplexity and number of codes in use, the codes revived by the last revival and in total.
        The only call here that synchronises with the device."""
        u, r = self.usage_stats.tolist(), self.revive_stats.tolist()
        return dict(perplexity=float(u[0]), codes_in_batch=int(u[1]), revived_last=int(r[0]), revived_total=int(r[1]), steps=self.steps,
                    events=self.events)
