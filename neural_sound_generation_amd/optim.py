"""Flat-bucket Adam: every parameter of the model lives in ONE contiguous fp32 buffer (each tensor
256-byte aligned inside it), gradients in a second one, so the optimiser is a single kernel launch
(nsg_adam_step) and data-parallel training needs a single all-reduce per step.

Arithmetic = torch.optim.Adam defaults as constructed at src/main.py:124 (no weight decay, no
amsgrad), applied element-wise, so the update is identical to the per-tensor optimiser's.

What the reference's training configuration names beyond that (src/hparams.py:105-118: lr_schedule, weight_decay,
clip_thresh, exponential_moving_average / ema_decay) is optional here and folds into the same step: one reduction over the
bucket (nsg_grad_sumsq) and one extended launch (nsg_adamw_step).  With every option at its default the step is the plain
nsg_adam_step call, bit for bit.
"""
from __future__ import annotations

import contextlib
import math

import torch

from . import ops

_ALIGN = 64  # floats (256 bytes): keeps every view 16-byte aligned for the float4 kernels


# ---- learning-rate schedules: callables step (1-based) -> multiplier of the group's lr -------------------------------
# The reference names the first two (src/hparams.py:106-107) but does not ship its lrschedule.py; these are the
# well-known forms of r9y9's wavenet_vocoder, which that configuration was taken from.
def noam_learning_rate_decay(warmup_steps: int = 4000):
    """lr * w^0.5 * min(s * w^-1.5, s^-0.5): linear warm-up to lr at step w, then lr * sqrt(w / s)."""
    w = float(warmup_steps)
    if not w >= 1:
        raise ValueError("noam_learning_rate_decay: warmup_steps must be >= 1")
    return lambda step: w ** 0.5 * min(step * w ** -1.5, step ** -0.5)


def step_learning_rate_decay(anneal_rate: float = 0.5, anneal_interval: int = 50000):
    """lr * anneal_rate^(s // anneal_interval)."""
    if int(anneal_interval) < 1:
        raise ValueError("step_learning_rate_decay: anneal_interval must be >= 1")
    return lambda step: float(anneal_rate) ** (int(step) // int(anneal_interval))


def warmup_cosine(warmup_steps: int, total_steps: int, floor: float = 0.0):
    """Linear warm-up to lr over warmup_steps, then half a cosine down to floor * lr at total_steps (and floor after)."""
    w, t = int(warmup_steps), int(total_steps)
    if w < 0 or t <= w:
        raise ValueError("warmup_cosine: need 0 <= warmup_steps < total_steps")

    def mult(step):
        if step <= w:
            return step / w
        x = min(1.0, (step - w) / (t - w))
        return floor + (1.0 - floor) * 0.5 * (1.0 + math.cos(math.pi * x))
    return mult


class FlatAdam(torch.optim.Optimizer):
    """Adam / AdamW over one flat bucket.  Options (all off by default; with all of them off step() is nsg_adam_step):

    weight_decay, no_decay   decoupled decay as torch.optim.AdamW.  Exempt: every tensor with ndim < 2 (biases, BatchNorm
                             gamma / beta) and, in addition, the tensors listed in no_decay -- the codebook is 2-D, so a VQ-VAE
                             passes no_decay=[model.codebook.embedding.weight].
    max_grad_norm            clip the global gradient norm as torch.nn.utils.clip_grad_norm_, on the device (no host sync).
                             In data parallel the norm is taken after the all-reduce and includes grad_scale = 1/R, so it is
                             the averaged gradient's and identical on every rank.  Only the gradients enter it, not a
                             reserved tail.
    skip_nonfinite           a step whose gradient norm is inf / NaN leaves parameters, moments and the shadow untouched.
                             The HOST's step count still advances (the kernel's decision never reaches the host), so the
                             bias correction of later steps sees one step more per skipped step.
    weight_ema_decay         keep shadow <- shadow - (1 - decay) (shadow - p) after every step (src/dataloader.py:246-267);
                             ema_weights() swaps it in.  (Not `ema_decay`: VQVAE(ema_decay=) is the codebook's EMA.)  BatchNorm
                             running statistics are buffers and are not averaged.  A code row re-seeded by CodebookReviver
                             keeps its old shadow row, which then converges to the new one at rate 1 - decay.
    lr_schedule              callable step (1-based) -> multiplier of the group's lr, evaluated on the host each step
                             (noam_learning_rate_decay, step_learning_rate_decay, warmup_cosine).  Code: not checkpointed.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, weight_decay=0.0, no_decay=None, max_grad_norm=None,
                 skip_nonfinite=False, weight_ema_decay=None, lr_schedule=None):
        params = [p for p in params if p.requires_grad]   # e.g. an EMA-trained codebook takes no gradient step
        if weight_decay < 0:
            raise ValueError("FlatAdam: weight_decay must be >= 0")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("FlatAdam: max_grad_norm must be > 0 (None = no clipping)")
        if weight_ema_decay is not None and not 0.0 <= weight_ema_decay <= 1.0:
            raise ValueError("FlatAdam: weight_ema_decay must lie in [0, 1]")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._params = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise ValueError("FlatAdam got no parameters")
        dev = self._params[0].device
        offs, total = [], 0
        for p in self._params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatAdam needs float32 parameters on one device")
            offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.offsets, self.total = offs, total
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad_views = []
        with torch.no_grad():
            for p, off in zip(self._params, offs):
                view = self.flat_param[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view                      # parameters now alias the flat buffer
                gview = self.flat_grad[off:off + p.numel()].view_as(p)
                p.grad = gview                     # autograd accumulates in place into the bucket
                self.grad_views.append(gview)
        self.flat_comm = self.flat_grad          # what a data-parallel step all-reduces: [gradients | reserved tail]
        self.step_count = 0
        # ---- the options ----
        listed = {id(t) for t in (no_decay or ())}
        unknown = listed - {id(p) for p in self._params}
        if unknown:
            raise ValueError("FlatAdam: no_decay lists %d tensor(s) that are not among the parameters" % len(unknown))
        self.no_decay = [i for i, p in enumerate(self._params) if p.ndim < 2 or id(p) in listed]
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.weight_ema_decay = None if weight_ema_decay is None else float(weight_ema_decay)
        self.lr_schedule = lr_schedule
        self.last_lr = float(lr)
        self.seg_end = self.seg_wd = None
        self._build_segments()
        # the shadow starts as the weights (clone_as_averaged_model's starting point); padding stays zero like the bucket's
        self.shadow = self.flat_param.clone() if self.weight_ema_decay is not None else None
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self._stats = torch.zeros(4, dtype=torch.int32, device=dev)       # float norm, float coef, int finite, int skipped

    def segment_table(self):
        """(ends, decays): one segment per parameter tensor, ending where the next tensor's 64-float-aligned view starts
        (the last at `total`), with the group's weight_decay or 0.0 for an exempt tensor.  Host lists."""
        wd = float(self.param_groups[0]["weight_decay"])
        exempt = set(self.no_decay)
        return self.offsets[1:] + [self.total], [0.0 if i in exempt else wd for i in range(len(self._params))]

    def _build_segments(self):
        self._table_wd = float(self.param_groups[0]["weight_decay"])      # the decay the device table was built for
        if self._table_wd == 0.0:
            self.seg_end = self.seg_wd = None
            return
        ends, wds = self.segment_table()
        dev = self.flat_param.device
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.seg_wd = torch.tensor(wds, dtype=torch.float32, device=dev)

    @property
    def plain(self) -> bool:
        """True when no option is on: step() then makes the plain adam_step call."""
        return (self.seg_end is None and self.max_grad_norm is None and not self.skip_nonfinite and self.shadow is None
                and self.lr_schedule is None)

    @torch.no_grad()
    def reserve_tail(self, n_floats: int) -> torch.Tensor:
        """Room for `n_floats` fp32 values BEHIND the gradients in the same allocation: per-step statistics that must be
        summed over ranks (the EMA codebook's per-code counts and sums) then ride in the gradients' one all-reduce
        (SURVEY.md section 8e).  Re-binds every p.grad to the new storage; returns the tail view."""
        pad = (int(n_floats) + _ALIGN - 1) // _ALIGN * _ALIGN
        comm = torch.zeros(self.total + pad, dtype=torch.float32, device=self.flat_grad.device)
        comm[:self.total].copy_(self.flat_grad)
        self.flat_comm = comm
        self.flat_grad = comm[:self.total]
        self.grad_views = []
        for p, off in zip(self._params, self.offsets):
            gview = self.flat_grad[off:off + p.numel()].view_as(p)
            p.grad = gview
            self.grad_views.append(gview)
        return comm[self.total:self.total + int(n_floats)]

    def zero_grad(self, set_to_none: bool = False):
        # the views must survive: never set to None
        self.flat_grad.zero_()
        for p, g in zip(self._params, self.grad_views):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def grads_for(self, tensors):
        """Bucket views for the given parameter tensors (same order)."""
        index = {id(p): i for i, p in enumerate(self._params)}
        return [self.grad_views[index[id(t)]] for t in tensors]

    # ---- checkpoint interchange (src/main.py:216-220 saves optimizer.state_dict()) -------------------
    # Same layout as torch.optim.Adam's / AdamW's: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]}
    # with weight_decay in the group, so a checkpoint written with either optimiser loads into the other.  Two extra
    # top-level keys, which torch's load_state_dict ignores: 'no_decay' (indices of the exempt parameters) and 'weight_ema'
    # ({'decay', 'shadow': [tensor per parameter]}, present only with weight_ema_decay).  The schedule is code: not saved.
    def state_dict(self):
        g = self.param_groups[0]
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)   # every key torch's Adam expects in a group
        group = {**defaults, "lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "params": list(range(len(self._params)))}
        if g["weight_decay"]:
            group["weight_decay"] = g["weight_decay"]
            if "decoupled_weight_decay" in defaults:
                group["decoupled_weight_decay"] = True                 # (torch.optim.Adam then decays as AdamW does)
        state = {}
        if self.step_count > 0:
            for i, (p, off) in enumerate(zip(self._params, self.offsets)):
                n = p.numel()
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.exp_avg[off:off + n].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[off:off + n].view_as(p).clone()}
        sd = {"state": state, "param_groups": [group]}
        if g["weight_decay"]:
            sd["no_decay"] = list(self.no_decay)
        if self.shadow is not None:
            sd["weight_ema"] = {"decay": self.weight_ema_decay,
                                "shadow": [self.shadow[off:off + p.numel()].view_as(p).clone() for p, off in zip(self._params, self.offsets)]}
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatAdam.load_state_dict: expected one parameter group with %d parameters" % len(self._params))
        if groups[0].get("amsgrad", False):
            raise ValueError("FlatAdam.load_state_dict: amsgrad is not implemented")
        wd = float(groups[0].get("weight_decay", 0) or 0)
        if wd and not groups[0].get("decoupled_weight_decay", True):
            raise ValueError("FlatAdam.load_state_dict: coupled (L2) weight decay is not implemented, only AdamW's decoupled decay")
        g = self.param_groups[0]
        g["lr"], g["betas"], g["eps"], g["weight_decay"] = groups[0]["lr"], tuple(groups[0]["betas"]), groups[0]["eps"], wd
        if "no_decay" in sd:
            idx = sorted(int(i) for i in sd["no_decay"])
            if idx and not 0 <= idx[0] <= idx[-1] < len(self._params):
                raise ValueError("FlatAdam.load_state_dict: no_decay index out of range")
            self.no_decay = idx
        self._build_segments()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = set()
        for i, (p, off) in enumerate(zip(self._params, self.offsets)):
            st = sd["state"].get(i)
            if st is None:
                continue
            n = p.numel()
            self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("FlatAdam.load_state_dict: parameters carry different step counts")
        self.step_count = steps.pop() if steps else 0
        ema = sd.get("weight_ema")
        if ema is not None:
            if len(ema["shadow"]) != len(self._params):
                raise ValueError("FlatAdam.load_state_dict: weight_ema holds %d tensors for %d parameters" % (len(ema["shadow"]), len(self._params)))
            if self.shadow is None:
                self.shadow = torch.zeros_like(self.flat_param)
            if self.weight_ema_decay is None:
                self.weight_ema_decay = float(ema["decay"])
            for p, off, s in zip(self._params, self.offsets, ema["shadow"]):
                self.shadow[off:off + p.numel()].copy_(s.reshape(-1))
        elif self.shadow is not None:
            self.shadow.copy_(self.flat_param)        # a checkpoint without a shadow: the average restarts from the weights in place

    def _lr_now(self, step: int) -> float:
        lr = self.param_groups[0]["lr"]
        return lr if self.lr_schedule is None else lr * float(self.lr_schedule(step))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        self.step_count += 1
        if float(g["weight_decay"]) != self._table_wd:
            self._build_segments()           # param_groups[0]['weight_decay'] was assigned since: the usual torch idiom
        if self.flat_param.is_cuda:
            if self.plain:
                ops.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_count, lr=g["lr"],
                              beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], grad_scale=grad_scale)
            else:
                self.last_lr = self._lr_now(self.step_count)
                need_norm = self.max_grad_norm is not None or self.skip_nonfinite
                if need_norm:
                    ops.grad_sumsq(self.flat_grad, out=self._sumsq)      # flat_grad is [:total] of the communication buffer
                ops.adamw_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.last_lr,
                               beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], grad_scale=grad_scale,
                               seg_end=self.seg_end, seg_wd=self.seg_wd, sumsq=self._sumsq if need_norm else None,
                               max_norm=self.max_grad_norm or 0.0, skip_nonfinite=self.skip_nonfinite, shadow=self.shadow,
                               one_minus_decay=0.0 if self.shadow is None else 1.0 - self.weight_ema_decay, stats=self._stats)
            # the kernel updated the parameters through raw pointers: bump autograd's version counters (each Parameter keeps its
            # own, `p.data = view` does not share the bucket's), so a backward through a graph built BEFORE this step raises
            # instead of differentiating against new values
            torch.autograd.graph.increment_version(self._params)
        else:
            raise RuntimeError("FlatAdam.step: parameters are not on a GPU; this path has no CPU fallback")
        return loss

    def stats(self) -> dict:
        """{'grad_norm', 'clip_coef', 'skipped_steps', 'lr'} of the last step, for logging: synchronises with the device.
        grad_norm / clip_coef are None when neither clipping nor the guard is on (the norm is then not taken)."""
        lr = self.param_groups[0]["lr"] if self.plain else self.last_lr
        if not self.flat_param.is_cuda or self.step_count == 0:
            return {"grad_norm": None, "clip_coef": None, "skipped_steps": 0, "lr": lr}
        norm, coef, _, skipped = ops.read_adamw_stats(self._stats)
        measured = self.max_grad_norm is not None or self.skip_nonfinite
        return {"grad_norm": norm if measured else None, "clip_coef": coef if measured else None, "skipped_steps": skipped, "lr": lr}

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters hold the averaged weights (the bucket's contents and the shadow are swapped);
        the raw weights are back on exit, exceptions included.  BatchNorm running statistics are buffers: they are NOT
        averaged, the block sees the raw model's.  Do not step inside the block."""
        if self.shadow is None:
            raise RuntimeError("FlatAdam.ema_weights: built without weight_ema_decay")
        self._swap_shadow()
        try:
            yield self
        finally:
            self._swap_shadow()

    @torch.no_grad()
    def _swap_shadow(self):
        tmp = self.flat_param.clone()
        self.flat_param.copy_(self.shadow)
        self.shadow.copy_(tmp)
        torch.autograd.graph.increment_version(self._params)      # as step(): the parameters changed under autograd
