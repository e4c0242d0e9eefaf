"""Tensor-level wrappers over the C ABI: validate, allocate outputs/workspaces as torch tensors
(so the caching allocator and stream semantics apply), pass raw pointers + the current HIP stream.
PyTorch is plumbing here: device memory, streams, autograd glue -- all arithmetic is in libnsg.so.
All activations are fp32 NHWC; see include/nsg.h.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import byref, c_void_p
from typing import NamedTuple

import torch

from . import _lib
from ._lib import ConvDesc, NSG_RELU_IN, NSG_TANH_OUT, NSG_OUT_F32, NSG_RELU_OUT, NSG_F32, NSG_BF16  # noqa: F401

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def nsg_dtype(torch_dtype) -> int:
    if torch_dtype == torch.float32:
        return NSG_F32
    if torch_dtype == torch.bfloat16:
        return NSG_BF16
    raise _lib.NsgError(f"unsupported activation dtype {torch_dtype} (float32 or bfloat16)")


def torch_dtype(nsg: int):
    return torch.bfloat16 if nsg == NSG_BF16 else torch.float32


def _chk(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.NsgError(f"{name}: expected a GPU tensor (this path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise _lib.NsgError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.NsgError(f"{name}: expected a contiguous tensor")
    return t


class Workspace:
    """One growing scratch buffer per (device, stream): kernels on one stream run in order, so reuse is safe; a second stream
    (engine.py runs the weight gradients on one) gets a buffer of its own."""

    def __init__(self):
        self._buf = {}

    @staticmethod
    def _key(device):
        sid = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        return (device.type, device.index, sid)

    def get(self, nbytes: int, device) -> torch.Tensor:
        key = self._key(device)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf

    def current(self, device):
        """The buffer get() hands out for `device` on the current stream right now (None before first use).  Growth REPLACES
        it; whoever baked its address into a HIP graph keeps a reference to this tensor so the address stays theirs
        (FusedTrainStep.capture)."""
        return self._buf.get(self._key(device))


WS = Workspace()


def _ws(device, query, *args):
    """(workspace on `device`, its size in bytes) as the size query `query` of an entry point asks for `args`."""
    nb = _lib.query(query, *args)
    return WS.get(nb, device), nb


class KernelTimer:
    """Optional HIP-event timing of the single-kernel GEMM launches (bench.py's roofline figure).
    Events are recorded on the stream the kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = {}   # name -> list of (start_event, end_event, flops)

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, name, start, flops, nbytes=0.0):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.setdefault(name, []).append((start, ev, flops, nbytes))

    def summary(self):
        """name -> dict(launches, total_ms, avg_ms, flops_per_launch, bytes_per_launch, tflops, tbps)  (call after a synchronize)"""
        out = {}
        for name, recs in self.records.items():
            ms = [r[0].elapsed_time(r[1]) for r in recs]
            tot_ms, tot_fl, tot_b = sum(ms), float(sum(r[2] for r in recs)), float(sum(r[3] for r in recs))
            out[name] = dict(launches=len(recs), total_ms=tot_ms, avg_ms=tot_ms / len(recs),
                             flops_per_launch=tot_fl / len(recs), bytes_per_launch=tot_b / len(recs),
                             tflops=tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0,
                             tbps=tot_b / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0)
        return out


KERNEL_TIMER = None  # set to a KernelTimer() to time gather_gemm / wgrad launches


def _es(t) -> int:
    return t.element_size()


def _conv_label(d: "ConvDesc", role: str) -> str:
    """Kernel + geometry label for the census: which gather_gemm mode a forward / dgrad of this layer runs (a transposed conv's
    forward and a stride-2 conv's data gradient are the 4-parity-class form, MODE 1; everything else is the conv gather, MODE 0).
    (As before for every stride-2 transposed layer: mode1 = transposed; the stride-1 transposed kind runs MODE 0.)"""
    kw = d.k_w if d.k_w > 0 else d.k
    geom = f"{d.k}x{kw}" + (f"/s{d.stride}" if d.stride != 1 else "")
    if role == "wgrad":
        return f"wgrad_gemm {geom}{' transposed' if d.transposed else ''} {d.C_in}->{d.C_out}"
    mode1 = (bool(d.transposed) if role == "forward" else not d.transposed) and d.stride == 2      # (stride-1 transposed: MODE 0 both ways)
    return f"gather_gemm MODE {1 if mode1 else 0} {geom} {role} {d.C_in}->{d.C_out}"


def _gemm_flops(d: "ConvDesc") -> float:
    """Algorithmic FLOPs of one forward / dgrad / wgrad of layer d: 2 * low-res pixels * k^2 * C_in * C_out."""
    low = d.B * (d.IH * d.IW if d.transposed else d.OH * d.OW)
    return 2.0 * low * d.k * (d.k_w if d.k_w > 0 else d.k) * d.C_in * d.C_out


# ------------------------------------------------------------------------------------------------
# vector quantiser
# ------------------------------------------------------------------------------------------------
class BnResRows(NamedTuple):
    """(N, D) rows given as their sources: z = bn_apply(h, mean, invstd, gamma, beta, residual=r, out_dtype=float32) WITHOUT
    that pass -- h, r bf16 (N, D), the four vectors fp32 (D,).  vq_forward (impl="bf16x3"), vq_losses_indexed and
    index_add_rows (impl="sorted") take one in place of the fp32 rows and return bit for bit what they return on them
    (include/nsg.h, the *_bnres entry points)."""
    h: torch.Tensor
    r: torch.Tensor
    mean: torch.Tensor
    invstd: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor

    @property
    def shape(self):
        return self.h.shape

    @property
    def device(self):
        return self.h.device

    def check(self, who):
        _chk(self.h, who + ": h", torch.bfloat16); _chk(self.r, who + ": r", torch.bfloat16)
        if self.h.dim() != 2 or self.r.shape != self.h.shape:
            raise _lib.NsgError(f"{who}: h and r must be (N, D) tensors of one shape")
        for v, name in ((self.mean, "mean"), (self.invstd, "invstd"), (self.gamma, "gamma"), (self.beta, "beta")):
            if _chk(v, f"{who}: {name}").numel() != self.h.shape[1]:
                raise _lib.NsgError(f"{who}: {name} must hold one value per column")
        return self

    def pointers(self):
        return tuple(_p(v) for v in self)


def bnres_rows_supported(D) -> bool:
    """Row widths all three consumers of a BnResRows take (the search stops at D = 256; the segment sum wants a power of two)."""
    return 8 <= D <= 256 and D & (D - 1) == 0


def vq_forward(x2d, codebook, want_codes=True, want_dist=False, impl="mfma", codes_bf16=None, clip_rows=None):
    """x2d (N,D), codebook (K,D) -> idx (N,) int64 [, codes (N,D)] [, dmin (N,)]
    impl: "mfma" = the bit-exact fp32 search (parity mode); "valu" = its vector-ALU cross-check; "bf16x3" = the bf16
    mode's search on the bf16 matrix pipe with split operands (relative distance error ~2^-16: near-ties may differ).
    codes_bf16 ("plain" | "relu", bf16x3 only): also return the code rows as a bf16 (N,D) tensor (ReLU'd: the decoder's
    input after its leading ReLU) as a 4th result.  clip_rows (B, D) fp32 (with codes_bf16): a per-clip conditioning row added
    to every bf16 code row of that clip before the ReLU (N = B * rows per clip; the speaker-conditioned decoder)."""
    bnres = isinstance(x2d, BnResRows)
    if bnres:
        x2d.check("vq_forward")
        if impl != "bf16x3" or want_codes or want_dist or not bnres_rows_supported(x2d.shape[1]):
            raise _lib.NsgError("vq_forward: rows given as their sources need impl='bf16x3', no fp32 codes or distances, D a power of two <= 256")
    else:
        _chk(x2d, "x")
    _chk(codebook, "codebook")
    if clip_rows is not None:
        _chk(clip_rows, "clip_rows")
        if impl != "bf16x3" or not codes_bf16 or clip_rows.shape[1] != x2d.shape[1] or x2d.shape[0] % clip_rows.shape[0] != 0:
            raise ValueError("vq_forward: clip_rows needs impl='bf16x3', codes_bf16 and (B, D) rows with N a multiple of B")
    N, D = x2d.shape
    K, D2 = codebook.shape
    if D != D2:
        raise _lib.NsgError(f"vq_forward: input rows have {D} columns, codebook has {D2}")
    idx = torch.empty(N, dtype=torch.int64, device=x2d.device)
    codes = torch.empty_like(x2d) if want_codes else None           # (never with BnResRows)
    dmin = torch.empty(N, dtype=torch.float32, device=x2d.device) if want_dist else None
    if N > 0:
        wsfn = "nsg_vq_bf16x3_workspace_bytes" if impl == "bf16x3" else "nsg_vq_workspace_bytes"
        ws, nb = _ws(x2d.device, wsfn, N, D, K)
        fn = {"mfma": "nsg_vq_forward", "valu": "nsg_debug_vq_forward_valu", "bf16x3": "nsg_vq_forward_bf16x3"}[impl]
        if impl == "bf16x3":
            lp = torch.empty(N, D, dtype=torch.bfloat16, device=x2d.device) if codes_bf16 else None
            _lib.tag("vq_forward_bf16x3 (search + gather)", 2.0 * N * K * D)
            if bnres:
                _lib.call("nsg_vq_forward_bf16x3_bnres", *x2d.pointers(), _p(codebook), N, D, K, _p(idx), _p(None), _p(lp),
                          1 if codes_bf16 == "relu" else 0, _p(clip_rows), N // clip_rows.shape[0] if clip_rows is not None else 0, _p(ws), nb,
                          _stream())
            elif clip_rows is not None:
                _lib.call("nsg_vq_forward_bf16x3_cond", _p(x2d), _p(codebook), N, D, K, _p(idx), _p(codes), _p(dmin), _p(lp),
                          1 if codes_bf16 == "relu" else 0, _p(clip_rows), N // clip_rows.shape[0], _p(ws), nb, _stream())
            else:
                _lib.call(fn, _p(x2d), _p(codebook), N, D, K, _p(idx), _p(codes), _p(dmin), _p(lp), 1 if codes_bf16 == "relu" else 0, _p(ws), nb,
                          _stream())
            if codes_bf16:
                return idx, codes, dmin, lp
            return idx, codes, dmin
        if codes_bf16:
            raise ValueError("vq_forward: codes_bf16 needs impl='bf16x3'")
        _lib.tag("vq_forward (fp32 exact search + gather)", 2.0 * N * K * D)
        _lib.call(fn, _p(x2d), _p(codebook), N, D, K, _p(idx), _p(codes), _p(dmin), _p(ws), nb, _stream())
    elif codes_bf16:
        return idx, codes, dmin, torch.empty(0, D, dtype=torch.bfloat16, device=x2d.device)
    return idx, codes, dmin


def rowsumsq(v):
    _chk(v, "v")
    out = torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    _lib.call("nsg_rowsumsq", _p(v), v.shape[0], v.shape[1], _p(out), _stream())
    return out


def index_add_sorted_supported(N, D, K) -> bool:
    """Shapes nsg_index_add_rows_sorted takes (include/nsg.h)."""
    ppr = D // 4
    return D % 4 == 0 and K <= 8192 and N < 2 ** 31 and (ppr > 64 and D % 256 == 0 or ppr <= 64 and ppr & (ppr - 1) == 0)


def index_add_rows(idx, g2d, K, want_counts=False, impl="f32", out=None, counts=None):
    """out[k] = sum of rows of g2d whose idx == k; deterministic.  impl: "sorted" (a sorted segment sum in fp32: N*D*4 bytes
    moved; the training step's default), "f32" (one-hot GEMM on the fp32 matrix pipe, exact products) or "bf16x2" (one-hot GEMM
    on the bf16 pipe: rows split into bf16 hi + lo, relative error of a sum ~2^-17).
    A row whose index lies outside [0, K) (compared as the 64-bit value it is) adds to no sum and to no count, in every form.
    out (K, D) / counts (K,): optional preallocated fp32 destinations (e.g. views of a communication buffer)."""
    _chk(idx, "idx", torch.int64)
    bnres = isinstance(g2d, BnResRows)
    if bnres:
        g2d.check("index_add_rows")
        if impl != "sorted" or not bnres_rows_supported(g2d.shape[1]) or not index_add_sorted_supported(g2d.shape[0], g2d.shape[1], K):
            raise _lib.NsgError("index_add_rows: rows given as their sources need impl='sorted' and a shape it takes (D a power of two <= 256)")
    else:
        _chk(g2d, "g")
    N, D = g2d.shape
    if out is None:
        out = torch.empty(K, D, dtype=torch.float32, device=g2d.device)
    elif _chk(out, "out").shape != (K, D):
        raise _lib.NsgError(f"index_add_rows: out has shape {tuple(out.shape)}, expected {(K, D)}")
    if counts is not None:
        if _chk(counts, "counts").shape != (K,):
            raise _lib.NsgError(f"index_add_rows: counts has shape {tuple(counts.shape)}, expected {(K,)}")
        want_counts = True
    elif want_counts:
        counts = torch.empty(K, dtype=torch.float32, device=g2d.device)
    if impl == "sorted" and not index_add_sorted_supported(N, D, K):
        impl = "f32"
    if impl == "sorted":
        if N == 0:
            out.zero_()
            if counts is not None:
                counts.zero_()
            return (out, counts) if want_counts else out
        ws, nb = _ws(g2d.device, "nsg_index_add_sorted_workspace_bytes", N, D, K)
        _lib.tag("index_add_rows (sorted segment sum)", 0, 4.0 * N * D + 8.0 * N)     # (two bf16 sources = the fp32 rows' bytes)
        if bnres:
            _lib.call("nsg_index_add_rows_sorted_bnres", _p(idx), *g2d.pointers(), N, D, K, _p(out), _p(counts), _p(ws), nb, _stream())
            return (out, counts) if want_counts else out
        _lib.call("nsg_index_add_rows_sorted", _p(idx), _p(g2d), N, D, K, _p(out), _p(counts), _p(ws), nb, _stream())
        return (out, counts) if want_counts else out
    ws, nb = _ws(g2d.device, "nsg_index_add_workspace_bytes", N, D, K)
    _lib.tag("index_add_rows (one-hot GEMM, %s)" % impl, 2.0 * N * K * D, 4.0 * N * D + 8.0 * N)
    _lib.call("nsg_index_add_rows_bf16x2" if impl == "bf16x2" else "nsg_index_add_rows", _p(idx), _p(g2d), N, D, K, _p(out), _p(counts), _p(ws), nb,
              _stream())
    return (out, counts) if want_counts else out


def codebook_grad_from_sums(codebook, n, s, scale, out):
    """out[k] = scale * (n[k] * codebook[k] - s[k]): the codebook gradient of mse(codebook[idx], sg(z)) from the per-code
    counts n (K,) and sums s (K, D) of the rows z assigned to each code (index_add_rows(..., want_counts=True))."""
    _chk(codebook, "codebook"); _chk(n, "n"); _chk(s, "s"); _chk(out, "out")
    K, D = codebook.shape
    if n.numel() != K or s.numel() != K * D or out.numel() != K * D:
        raise _lib.NsgError("codebook_grad_from_sums: n, s and out must match the codebook's (K, D)")
    _lib.call("nsg_codebook_grad_from_sums", _p(codebook), _p(n), _p(s), K, D, scale, _p(out), _stream())
    return out


def code_usage(idx, K, window, stats=None, batch_counts=None):
    """Histogram of a batch's code indices (any shape, int64; indices outside [0, K) are ignored) -> (batch_counts (K,) int32,
    stats (2,) float64 = [the batch's perplexity, the number of codes in the batch]); window (K,) int32 += batch_counts.
    Nothing synchronises: the two tensors are device results."""
    _chk(idx, "idx", torch.int64); _chk(window, "window", torch.int32)
    K = int(K)
    if window.shape != (K,):
        raise _lib.NsgError(f"code_usage: window has shape {tuple(window.shape)}, expected {(K,)}")
    if batch_counts is None:
        batch_counts = torch.empty(K, dtype=torch.int32, device=idx.device)
    elif _chk(batch_counts, "batch_counts", torch.int32).shape != (K,):
        raise _lib.NsgError(f"code_usage: batch_counts has shape {tuple(batch_counts.shape)}, expected {(K,)}")
    if stats is None:
        stats = torch.empty(2, dtype=torch.float64, device=idx.device)
    elif _chk(stats, "stats", torch.float64).numel() != 2:
        raise _lib.NsgError("code_usage: stats must hold two float64 values")
    _lib.tag("code_usage (histogram + perplexity)", 0, 8.0 * idx.numel())
    _lib.call("nsg_code_usage", _p(idx), idx.numel(), K, _p(batch_counts), _p(window), _p(stats), _stream())
    return batch_counts, stats


def vq_revive(rows, codebook, window, min_count=1, base_row=0, stride=1, adam_m=None, adam_v=None, ema_count=None, ema_sum=None,
              slot=None, stats=None, revive_all=False):
    """Re-seed the dead codes of `codebook` (K, D) from `rows`, the current encoder output: (N, D) fp32 rows or a BnResRows.
    Code k is dead when window[k] < min_count (or revive_all); the j-th dead code, in index order, takes row
    (base_row + j * stride) mod N bit for bit; adam_m / adam_v (K, D) rows of dead codes are zeroed, ema_count (K,) / ema_sum
    (K, D) set to 1 / the row; live rows are not written; window is cleared (include/nsg.h, nsg_vq_revive).
    Returns (slot (K,) int32: j for a dead code, -1 for a live one; stats (2,) int64: [revived now, running total])."""
    bnres = isinstance(rows, BnResRows)
    if bnres:
        rows.check("vq_revive")
    else:
        _chk(rows, "rows")
        if rows.dim() != 2:
            raise _lib.NsgError("vq_revive: rows must be an (N, D) tensor")
    _chk(codebook, "codebook"); _chk(window, "window", torch.int32)
    N, D = rows.shape
    K = codebook.shape[0]
    if codebook.dim() != 2 or codebook.shape[1] != D or window.shape != (K,):
        raise _lib.NsgError(f"vq_revive: rows have {D} columns; codebook {tuple(codebook.shape)} and window {tuple(window.shape)} must be (K, {D}) and (K,)")
    for t, name, shape in ((adam_m, "adam_m", (K, D)), (adam_v, "adam_v", (K, D)), (ema_sum, "ema_sum", (K, D)), (ema_count, "ema_count", (K,))):
        if t is not None and _chk(t, "vq_revive: " + name).shape != shape:
            raise _lib.NsgError(f"vq_revive: {name} has shape {tuple(t.shape)}, expected {shape}")
    if slot is None:
        slot = torch.empty(K, dtype=torch.int32, device=codebook.device)
    elif _chk(slot, "slot", torch.int32).shape != (K,):
        raise _lib.NsgError(f"vq_revive: slot has shape {tuple(slot.shape)}, expected {(K,)}")
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int64, device=codebook.device)
    elif _chk(stats, "stats", torch.int64).numel() != 2:
        raise _lib.NsgError("vq_revive: stats must hold two int64 values")
    tail = (N, D, _p(codebook), K, _p(window), int(min_count), int(base_row), int(stride),
            _p(adam_m), _p(adam_v), _p(ema_count), _p(ema_sum), _p(slot), _p(stats), 1 if revive_all else 0, _stream())
    _lib.tag("vq_revive (dead-code re-seed)", 0, 8.0 * K * D)
    if bnres:
        _lib.call("nsg_vq_revive_bnres", *rows.pointers(), *tail)
    else:
        _lib.call("nsg_vq_revive", _p(rows), *tail)
    return slot, stats


def increment_counters(counters):
    """counters: int64 GPU scalars (BatchNorm2d.num_batches_tracked), each += 1, one launch."""
    n = len(counters)
    if n == 0:
        return
    arr = (c_void_p * n)()
    for i, t in enumerate(counters):
        if not t.is_cuda or t.dtype != torch.int64 or t.numel() != 1:
            raise _lib.NsgError("increment_counters: expected int64 GPU scalars")
        arr[i] = t.data_ptr()
    _lib.call("nsg_increment_counters", ctypes.cast(arr, c_void_p), n, _stream())


def gather_rows(codebook, idx, out=None):
    """codebook (K,D), idx (...) int64 -> (..., D)"""
    _chk(codebook, "codebook"); _chk(idx, "idx", torch.int64)
    K, D = codebook.shape
    if out is None:
        out = torch.empty(*idx.shape, D, dtype=torch.float32, device=codebook.device)
    elif _chk(out, "out").numel() != idx.numel() * D:
        raise _lib.NsgError(f"gather_rows: out {tuple(out.shape)} does not hold {idx.numel()} rows of {D}")
    _lib.call("nsg_gather_rows", _p(codebook), _p(idx), idx.numel(), D, K, _p(out), _stream())
    return out


COLLATE_MAX_MELS = 128


def check_collate_plan(plan, T, corpus_frames):
    """The precondition of nsg_collate_mels, checked where the plan is built: `plan` (..., 3) int64 ON THE HOST (a numpy array or
    a CPU tensor), rows (clip, start, count); `T` the width of the batch, or an array that broadcasts against plan[..., 0] (one
    width per batch of an epoch's plan).  Raises NsgError for start < 0, count outside [0, T] or start + count > corpus_frames."""
    import numpy as np
    p = plan.numpy() if isinstance(plan, torch.Tensor) else np.asarray(plan)
    if p.dtype != np.int64 or p.ndim < 1 or p.shape[-1] != 3:
        raise _lib.NsgError(f"collate plan: expected int64 rows of (clip, start, count), got {p.dtype} {p.shape}")
    start, count = p[..., 1], p[..., 2]
    if (start < 0).any():
        raise _lib.NsgError(f"collate plan: start < 0 (least {int(start.min())})")
    if (count < 0).any() or (count > np.asarray(T)).any():
        raise _lib.NsgError(f"collate plan: count outside [0, T] (counts {int(count.min())} .. {int(count.max())}, T = {T})")
    if (start + count > corpus_frames).any():
        raise _lib.NsgError(f"collate plan: start + count = {int((start + count).max())} is past the corpus' {corpus_frames} frames")


def collate_mels(corpus, plan, T, out=None):
    """corpus (frames, n_mels) fp32 frame-major, plan (B, 3) int64 rows of (clip, start, count), T -> (B, n_mels, T) mel-major:
    out[b, :, t] = corpus[start_b + t] for t < count_b, +0.0 up to T (data.Collate's crop, padding and transpose; one launch).
    A plan on the device is the caller's to have checked (check_collate_plan on its host copy: ResidentMelLoader checks an epoch's
    plan once, before the upload); a plan on the host is checked here and uploaded."""
    for t, name, dtype in ((corpus, "corpus", torch.float32), (plan, "plan", torch.int64)):
        if t.dtype != dtype:
            raise _lib.NsgError(f"collate_mels: {name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.NsgError(f"collate_mels: {name}: expected a contiguous tensor")
    if corpus.dim() != 2 or not 1 <= corpus.shape[1] <= COLLATE_MAX_MELS:
        raise _lib.NsgError(f"collate_mels: corpus {tuple(corpus.shape)} is not (frames, n_mels) with n_mels in [1, {COLLATE_MAX_MELS}]")
    if plan.dim() != 2 or plan.shape[1] != 3 or plan.shape[0] < 1:
        raise _lib.NsgError(f"collate_mels: plan {tuple(plan.shape)} is not (B, 3) with B >= 1")
    T = int(T)
    if T < 1:
        raise _lib.NsgError(f"collate_mels: T = {T} < 1")
    frames, n_mels = corpus.shape
    B = plan.shape[0]
    if not plan.is_cuda:
        check_collate_plan(plan, T, frames)
    _chk(corpus, "collate_mels: corpus")
    if not plan.is_cuda:
        plan = plan.to(corpus.device)
    if out is None:
        out = torch.empty(B, n_mels, T, dtype=torch.float32, device=corpus.device)
    elif _chk(out, "collate_mels: out").numel() != B * n_mels * T:
        raise _lib.NsgError(f"collate_mels: out {tuple(out.shape)} does not hold {B} x {n_mels} x {T}")
    _lib.call("nsg_collate_mels", _p(corpus), frames, n_mels, _p(plan), B, T, _p(out), _stream())
    return out


def collate_audio(corpus, plan, T, hop=256, out=None):
    """corpus (samples,) fp32: the clips' audio concatenated in the mel corpus' clip order, frames * hop samples a clip; plan (B, 3)
    int64, collate_mels' own rows (clip, start, count) in FRAMES; T -> (B, T * hop) fp32:
    out[b, i] = corpus[start_b * hop + i] for i < count_b * hop, +0.0 up to T * hop (data.Collate's audio crop and padding; one
    launch, a copy bit for bit).  The plan is checked as collate_mels checks it, against corpus.numel() // hop frames: on the host
    here, on the device by the caller on its host copy."""
    for t, name, dtype in ((corpus, "corpus", torch.float32), (plan, "plan", torch.int64)):
        if t.dtype != dtype:
            raise _lib.NsgError(f"collate_audio: {name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.NsgError(f"collate_audio: {name}: expected a contiguous tensor")
    if corpus.dim() != 1:
        raise _lib.NsgError(f"collate_audio: corpus {tuple(corpus.shape)} is not (samples,)")
    if plan.dim() != 2 or plan.shape[1] != 3 or plan.shape[0] < 1:
        raise _lib.NsgError(f"collate_audio: plan {tuple(plan.shape)} is not (B, 3) with B >= 1")
    T, hop = int(T), int(hop)
    if T < 1 or hop < 1 or T * hop >= 1 << 31:
        raise _lib.NsgError(f"collate_audio: T = {T}, hop = {hop}: both must be positive and T * hop below 2^31")
    B = plan.shape[0]
    if not plan.is_cuda:
        check_collate_plan(plan, T, corpus.numel() // hop)
    _chk(corpus, "collate_audio: corpus")
    if not plan.is_cuda:
        plan = plan.to(corpus.device)
    if out is None:
        out = torch.empty(B, T * hop, dtype=torch.float32, device=corpus.device)
    elif _chk(out, "collate_audio: out").numel() != B * T * hop:
        raise _lib.NsgError(f"collate_audio: out {tuple(out.shape)} does not hold {B} x {T * hop}")
    _lib.call("nsg_collate_audio", _p(corpus), corpus.numel(), hop, _p(plan), B, T, _p(out), _stream())
    return out


DTW_MAX_FRAMES, DTW_BLOCK_COLS =_lib.NSG_DTW_MAX_FRAMES, _lib.NSG_DTW_BLOCK_COLS     # include/nsg.h: longest sequence; columns of one sweep


def _lengths_on(lengths, name, B, lo, hi, device):
    """`lengths` as the (B,) int32 device tensor an entry point reads.  On the host (a sequence, a numpy array or a CPU tensor)
    they are checked against [lo, hi] here and uploaded; an int32 tensor already on the device is the caller's to have checked on
    the host copy it came from (include/nsg.h: the kernels clamp, so no access leaves a buffer)."""
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise _lib.NsgError(f"{name}: expected an int32 tensor of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        return _chk(lengths, name, torch.int32)
    import numpy as np
    host = lengths.numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
    if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer):
        raise _lib.NsgError(f"{name}: expected {B} integers, got {host.dtype} {host.shape}")
    if host.min() < lo or host.max() > hi:
        raise _lib.NsgError(f"{name}: every length must be in [{lo}, {hi}], got {int(host.min())} .. {int(host.max())}")
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(device)


def mel_cepstra(mel, table, frames=None, out=None):
    """mel (B, n_mels, T) fp32 mel-major, table (K, n_mels) fp32 -> (B, T, K) fp32 frame-major: c[b, t] = table @ mel[b, :, t] as
    one fp32 chain per output over the bands in order (include/nsg.h), +0.0 for t >= frames[b].  frames: None (all T), or (B,)
    lengths in [0, T] (host: checked here; int32 on the device: the caller's)."""
    _chk(mel, "mel_cepstra: mel"); _chk(table, "mel_cepstra: table")
    if mel.dim() != 3 or table.dim() != 2 or table.shape[1] != mel.shape[1] or table.device != mel.device:
        raise _lib.NsgError(f"mel_cepstra: mel {tuple(mel.shape)} / table {tuple(table.shape)} are not (B, n_mels, T) / (K, n_mels) on one device")
    B, n_mels, T = mel.shape
    K = table.shape[0]
    if B < 1 or T < 1:
        raise _lib.NsgError(f"mel_cepstra: empty mel {tuple(mel.shape)}")
    fr = None if frames is None else _lengths_on(frames, "mel_cepstra: frames", B, 0, T, mel.device)
    if out is None:
        out = torch.empty(B, T, K, dtype=torch.float32, device=mel.device)
    elif _chk(out, "mel_cepstra: out").numel() != B * T * K or out.device != mel.device:
        raise _lib.NsgError(f"mel_cepstra: out {tuple(out.shape)} does not hold {B} x {T} x {K}")
    _lib.call("nsg_mel_cepstra", _p(mel), _p(fr), _p(table), _p(out), B, n_mels, T, K, _stream())
    return out


def dtw(a, b, len_a, len_b, want_path=False, out=None):
    """Batched dynamic time warping (include/nsg.h: nsg_dtw).  a (B, Ta, K), b (B, Tb, K) fp32; len_a, len_b (B,) lengths in
    [1, Ta] / [1, Tb] (host: checked here and uploaded; int32 on the device: the caller's) -> cost (B,) fp32, steps (B,) int32 and,
    with want_path, path (B, Ta + Tb - 1, 2) int32 whose first steps[p] rows are pair p's cells (the rest is not written).  out: the
    result tensors to write instead of new ones, (cost, steps) or (cost, steps, path).  K and the
    sequence lengths the kernel serves are the entry point's to state and to refuse (K <= 64, Ta, Tb <= DTW_MAX_FRAMES)."""
    _chk(a, "dtw: a"); _chk(b, "dtw: b")
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or a.device != b.device:
        raise _lib.NsgError(f"dtw: a {tuple(a.shape)} / b {tuple(b.shape)} are not (B, Ta, K) / (B, Tb, K) on one device")
    B, Ta, K = a.shape
    Tb = b.shape[1]
    if B < 1 or Ta < 1 or Tb < 1:
        raise _lib.NsgError(f"dtw: empty a {tuple(a.shape)} or b {tuple(b.shape)}")
    la = _lengths_on(len_a, "dtw: len_a", B, 1, Ta, a.device)
    lb = _lengths_on(len_b, "dtw: len_b", B, 1, Tb, a.device)
    if out is None:
        cost = torch.empty(B, dtype=torch.float32, device=a.device)
        steps = torch.empty(B, dtype=torch.int32, device=a.device)
        path = torch.empty(B, Ta + Tb - 1, 2, dtype=torch.int32, device=a.device) if want_path else None
    else:
        cost, steps, path = out if want_path else (*out, None)
        for t, name, dtype, n in ((cost, "cost", torch.float32, B), (steps, "steps", torch.int32, B), (path, "path", torch.int32, B * (Ta + Tb - 1) * 2)):
            if t is not None and (_chk(t, f"dtw: out {name}", dtype).numel() != n or t.device != a.device):
                raise _lib.NsgError(f"dtw: out {name} {tuple(t.shape)} does not hold {n} elements")
    if not want_path:
        _lib.call("nsg_dtw", _p(a), _p(b), _p(la), _p(lb), _p(cost), _p(steps), None, B, Ta, Tb, K, None, 0, _stream())
        return cost, steps
    ws, nb = _ws(a.device, "nsg_dtw_workspace_bytes", B, Ta, Tb, 1)
    _lib.call("nsg_dtw", _p(a), _p(b), _p(la), _p(lb), _p(cost), _p(steps), _p(path), B, Ta, Tb, K, _p(ws), nb, _stream())
    return cost, steps, path


def f0(wav, frame_length, hop, tau_min, tau_max, threshold, sample_rate, lengths=None, out=None):
    """YIN F0 tracking (include/nsg.h: nsg_audio_f0).  wav (B, L) fp32 zero-padded clips; lengths: None (all L), or (B,) lengths
    in [0, L] (host: checked here and uploaded; int32 on the device: the caller's) -> (f0 (B, T), aperiodicity (B, T)) fp32,
    T = 1 + L // hop; f0 is +0.0 on unvoiced frames and past a clip's 1 + length // hop frames.  out: (f0, ap) to write instead of
    new tensors.  The frame length, lag range, threshold and rate the kernel serves are the entry point's to state and refuse."""
    _chk(wav, "f0: wav")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise _lib.NsgError(f"f0: wav {tuple(wav.shape)} is not (B, L) with B, L >= 1")
    B, L = wav.shape
    if int(hop) < 1:
        raise _lib.NsgError(f"f0: hop = {hop} < 1")
    T = 1 + L // int(hop)
    lens = None if lengths is None else _lengths_on(lengths, "f0: lengths", B, 0, L, wav.device)
    if out is None:
        f, ap = (torch.empty(B, T, dtype=torch.float32, device=wav.device) for _ in range(2))
    else:
        f, ap = out
        for t, name in ((f, "f0"), (ap, "ap")):
            if _chk(t, f"f0: out {name}").numel() != B * T or t.device != wav.device:
                raise _lib.NsgError(f"f0: out {name} {tuple(t.shape)} does not hold {B} x {T}")
    _lib.call("nsg_audio_f0", _p(wav), _p(lens), _p(f), _p(ap), B, L, int(frame_length), int(hop), int(tau_min), int(tau_max),
              float(threshold), float(sample_rate), _stream())
    return f, ap


F0_MAX_CANDIDATES = _lib.NSG_F0_MAX_CANDIDATES              # include/nsg.h: candidate slots of a frame
F0_VITERBI_LDS_FRAMES = _lib.NSG_F0_VITERBI_LDS_FRAMES      # include/nsg.h: beyond it nsg_f0_viterbi wants a workspace


def f0_candidates(wav, frame_length, hop, tau_min, tau_max, sample_rate, lengths=None, out=None):
    """The F0 candidates of every frame (include/nsg.h: nsg_audio_f0_candidates): the local minima of YIN's d' below 1, the 8
    strongest, by ascending lag.  wav (B, L) fp32 zero-padded clips; lengths as ops.f0 takes them -> (cand_f0, cand_ap, cand_logf
    (B, T, 8) fp32, count (B, T) int32), T = 1 + L // hop; slots past count hold (+0.0, 1.0, +0.0).  out: the four tensors to
    write instead of new ones."""
    _chk(wav, "f0_candidates: wav")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise _lib.NsgError(f"f0_candidates: wav {tuple(wav.shape)} is not (B, L) with B, L >= 1")
    B, L = wav.shape
    if int(hop) < 1:
        raise _lib.NsgError(f"f0_candidates: hop = {hop} < 1")
    T = 1 + L // int(hop)
    lens = None if lengths is None else _lengths_on(lengths, "f0_candidates: lengths", B, 0, L, wav.device)
    if out is None:
        cf, ca, cl = (torch.empty(B, T, F0_MAX_CANDIDATES, dtype=torch.float32, device=wav.device) for _ in range(3))
        cnt = torch.empty(B, T, dtype=torch.int32, device=wav.device)
    else:
        cf, ca, cl, cnt = out
        for t, name, dtype, n in ((cf, "cand_f0", torch.float32, B * T * F0_MAX_CANDIDATES), (ca, "cand_ap", torch.float32, B * T * F0_MAX_CANDIDATES),
                                  (cl, "cand_logf", torch.float32, B * T * F0_MAX_CANDIDATES), (cnt, "count", torch.int32, B * T)):
            if _chk(t, f"f0_candidates: out {name}", dtype).numel() != n or t.device != wav.device:
                raise _lib.NsgError(f"f0_candidates: out {name} {tuple(t.shape)} does not hold {n} elements")
    _lib.call("nsg_audio_f0_candidates", _p(wav), _p(lens), _p(cf), _p(ca), _p(cl), _p(cnt), B, L, int(frame_length), int(hop), int(tau_min),
              int(tau_max), float(sample_rate), _stream())
    return cf, ca, cl, cnt


def f0_viterbi(cand_logf, cand_ap, cand_f0, count, logf_top, octave_cost, jump_cost, vuv_cost, unvoiced_cost, frames=None, out=None):
    """The min-sum path over candidate tensors (include/nsg.h: nsg_f0_viterbi).  cand_logf, cand_ap, cand_f0 (B, T, 8) fp32, count
    (B, T) int32 (clamped into [0, 8] by the kernel); frames: None (all T), or (B,) frame counts in [0, T] (host: checked here and
    uploaded; int32 on the device: the caller's) -> (state (B, T) int32, cost (B,) fp32, f0 (B, T), ap (B, T) fp32).  State 0 is
    unvoiced, k >= 1 is slot k - 1, -1 is past the clip.  out: the four tensors to write instead of new ones."""
    for t, name in ((cand_logf, "cand_logf"), (cand_ap, "cand_ap"), (cand_f0, "cand_f0")):
        _chk(t, f"f0_viterbi: {name}")
    _chk(count, "f0_viterbi: count", torch.int32)
    if cand_logf.dim() != 3 or cand_logf.shape[0] < 1 or cand_logf.shape[1] < 1 or cand_logf.shape[2] != F0_MAX_CANDIDATES:
        raise _lib.NsgError(f"f0_viterbi: cand_logf {tuple(cand_logf.shape)} is not (B, T, {F0_MAX_CANDIDATES}) with B, T >= 1")
    B, T, _ = cand_logf.shape
    if cand_ap.shape != cand_logf.shape or cand_f0.shape != cand_logf.shape or tuple(count.shape) != (B, T):
        raise _lib.NsgError(f"f0_viterbi: cand_ap {tuple(cand_ap.shape)} / cand_f0 {tuple(cand_f0.shape)} / count {tuple(count.shape)} do not go "
                            f"with cand_logf {tuple(cand_logf.shape)}")
    if len({t.device for t in (cand_logf, cand_ap, cand_f0, count)}) != 1:
        raise _lib.NsgError("f0_viterbi: the tensors are not on one device")
    dev = cand_logf.device
    fr = None if frames is None else _lengths_on(frames, "f0_viterbi: frames", B, 0, T, dev)
    if out is None:
        state = torch.empty(B, T, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        f, ap = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(2))
    else:
        state, cost, f, ap = out
        for t, name, dtype, n in ((state, "state", torch.int32, B * T), (cost, "cost", torch.float32, B), (f, "f0", torch.float32, B * T),
                                  (ap, "ap", torch.float32, B * T)):
            if _chk(t, f"f0_viterbi: out {name}", dtype).numel() != n or t.device != dev:
                raise _lib.NsgError(f"f0_viterbi: out {name} {tuple(t.shape)} does not hold {n} elements")
    nb = _lib.query("nsg_f0_viterbi_workspace_bytes", B, T)
    ws = WS.get(nb, dev) if nb else None
    _lib.call("nsg_f0_viterbi", _p(cand_logf), _p(cand_ap), _p(cand_f0), _p(count), _p(fr), _p(state), _p(cost), _p(f), _p(ap), B, T,
              float(logf_top), float(octave_cost), float(jump_cost), float(vuv_cost), float(unvoiced_cost), _p(ws), nb, _stream())
    return state, cost, f, ap


def f0_path_stats(f0_a, f0_b, path, steps, out=None):
    """F0 statistics along warping paths (include/nsg.h: nsg_f0_path_stats).  f0_a (B, Ta), f0_b (B, Tb) fp32 (not > 0: unvoiced),
    path (B, Ta + Tb - 1, 2) int32 and steps (B,) int32 as ops.dtw returns them -> stats (B, 10) fp64:
    steps, n_vv, n_a_only, n_b_only, sum x, sum y, sum x^2, sum y^2, sum x y, sum (x - y)^2 with x, y = log2 f0 on the cells both voice."""
    _chk(f0_a, "f0_path_stats: f0_a"); _chk(f0_b, "f0_path_stats: f0_b")
    _chk(path, "f0_path_stats: path", torch.int32); _chk(steps, "f0_path_stats: steps", torch.int32)
    if f0_a.dim() != 2 or f0_b.dim() != 2 or f0_a.shape[0] != f0_b.shape[0] or f0_a.shape[0] < 1 or f0_a.shape[1] < 1 or f0_b.shape[1] < 1:
        raise _lib.NsgError(f"f0_path_stats: f0_a {tuple(f0_a.shape)} / f0_b {tuple(f0_b.shape)} are not (B, Ta) / (B, Tb)")
    B, Ta = f0_a.shape
    Tb = f0_b.shape[1]
    if tuple(path.shape) != (B, Ta + Tb - 1, 2) or tuple(steps.shape) != (B,):
        raise _lib.NsgError(f"f0_path_stats: path {tuple(path.shape)} / steps {tuple(steps.shape)} are not ({B}, {Ta + Tb - 1}, 2) / ({B},)")
    if len({t.device for t in (f0_a, f0_b, path, steps)}) != 1:
        raise _lib.NsgError("f0_path_stats: the tensors are not on one device")
    if out is None:
        out = torch.empty(B, 10, dtype=torch.float64, device=f0_a.device)
    elif _chk(out, "f0_path_stats: out", torch.float64).numel() != B * 10 or out.device != f0_a.device:
        raise _lib.NsgError(f"f0_path_stats: out {tuple(out.shape)} does not hold {B} x 10")
    _lib.call("nsg_f0_path_stats", _p(f0_a), _p(f0_b), _p(path), _p(steps), _p(out), B, Ta, Tb, _stream())
    return out


TEMPO_MAX_OVERLAP, TEMPO_MAX_SEGMENT, TEMPO_MAX_SEARCH = 2048, 8192, 2048     # include/nsg.h: nsg_audio_tempo's envelope
TEMPO_MIN_FACTOR, TEMPO_MAX_FACTOR = 0.25, 4.0


def tempo_out_lengths(lengths, factor):
    """out_lengths[b] = floor((double)lengths[b] / factor[b]) in fp64, as include/nsg.h states it (int64 numpy)."""
    import numpy as np
    return np.floor(np.asarray(lengths, dtype=np.float64) / np.asarray(factor, dtype=np.float64)).astype(np.int64)


def tempo(wav, factor, S, O, W, lengths=None, want_positions=False, out=None):
    """Waveform-similarity overlap-add (include/nsg.h: nsg_audio_tempo).  wav (B, L) fp32 zero-padded clips; factor: B finite
    numbers in [0.25, 4] on the host (above 1 is faster); lengths: None (all L) or B integers in [0, L] on the host -- the
    output lengths are formed from the host copies, which is why neither may be a device tensor -> (out (B, L_out) fp32 with
    +0.0 past each clip, out_lengths (B,) int32 numpy = floor(lengths / factor), L_out = max(1, max out_lengths)) and, with
    want_positions, positions (B, ceil(L_out / (S - O))) int32: each segment's start in the input, -1 past a clip's segments.
    out: the tensor to write instead of a new one, (B, L_out') with L_out' >= every out_length (it fixes L_out).  The segment
    sizes the kernel serves are the entry point's to state and refuse; everything the entry point cannot see is checked here."""
    import numpy as np
    _chk(wav, "tempo: wav")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise _lib.NsgError(f"tempo: wav {tuple(wav.shape)} is not (B, L) with B, L >= 1")
    B, L = wav.shape
    S, O, W = int(S), int(O), int(W)
    if O < 1 or S < 2 * O:
        raise _lib.NsgError(f"tempo: need 1 <= O and 2 O <= S, got S = {S}, O = {O}")
    f = np.asarray(factor, dtype=np.float64)
    f = np.array(np.broadcast_to(f, (B,)) if f.ndim == 0 else f)                 # a writable, contiguous copy
    if f.shape != (B,) or not np.isfinite(f).all() or f.min() < TEMPO_MIN_FACTOR or f.max() > TEMPO_MAX_FACTOR:
        raise _lib.NsgError(f"tempo: factor must be {B} finite number(s) in [{TEMPO_MIN_FACTOR}, {TEMPO_MAX_FACTOR}], got {factor!r}")
    if lengths is None:
        lens_h = None
    else:
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            raise _lib.NsgError("tempo: lengths must be on the host (the output lengths are formed from them)")
        lens_h = lengths.numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
        if lens_h.shape != (B,) or not np.issubdtype(lens_h.dtype, np.integer):
            raise _lib.NsgError(f"tempo: lengths: expected {B} integers, got {lens_h.dtype} {lens_h.shape}")
        if lens_h.min() < 0 or lens_h.max() > L:
            raise _lib.NsgError(f"tempo: lengths: every length must be in [0, {L}], got {int(lens_h.min())} .. {int(lens_h.max())}")
    out_lens = tempo_out_lengths(np.full(B, L, dtype=np.int64) if lens_h is None else lens_h, f)
    if out is None:
        L_out = max(1, int(out_lens.max()))
        if B * L_out >= 2 ** 31 - 1:
            raise _lib.NsgError(f"tempo: {B} clips of {L_out} output samples are 2^31 or more")
        out = torch.empty(B, L_out, dtype=torch.float32, device=wav.device)
    else:
        if _chk(out, "tempo: out").dim() != 2 or out.shape[0] != B or out.shape[1] < max(1, int(out_lens.max())) or out.device != wav.device:
            raise _lib.NsgError(f"tempo: out {tuple(out.shape)} does not hold {B} clips of up to {int(out_lens.max())} samples")
        L_out = out.shape[1]
    packed = np.empty(4 * B, dtype=np.int32)            # one upload: factor (fp64, first: 8-byte aligned) | out_lengths | lengths
    packed[:2 * B] = f.view(np.int32)
    packed[2 * B:3 * B] = out_lens
    packed[3 * B:] = 0 if lens_h is None else lens_h
    packed = torch.from_numpy(packed).to(wav.device)
    f_d, ol_d, lens_d = packed[:2 * B], packed[2 * B:3 * B], (None if lens_h is None else packed[3 * B:])
    M_max = -(-L_out // (S - O))
    pos = torch.empty(B, M_max, dtype=torch.int32, device=wav.device) if want_positions else None
    ws, nb = (None, 0) if want_positions else _ws(wav.device, "nsg_audio_tempo_workspace_bytes", B, L_out, S, O)
    _lib.call("nsg_audio_tempo", _p(wav), _p(lens_d), _p(f_d), _p(ol_d), _p(out), _p(pos), B, L, L_out, S, O, W, _p(ws), nb, _stream())
    res = (out, out_lens.astype(np.int32))
    return res + (pos,) if want_positions else res


PSOLA_MAX_PERIOD, PSOLA_MIN_HOP, PSOLA_MAX_HOP = 1024, 16, 2 ** 20      # include/nsg.h: nsg_audio_pitch_marks' envelope
PSOLA_MIN_WEIGHT = 2.0 ** -_lib.NSG_PSOLA_MIN_WEIGHT_LOG2               # below it the overlap-add passes the input through


def psola_sizes(L, P_min, P_max, alpha):
    """(G, K_max, H_max, G_s, J_max) of include/nsg.h for rows of L samples, periods [P_min, P_max] and alpha = (num, den): the
    least and (H_max) greatest distance of two marks, the marks a row can have, and the same for the synthesis marks."""
    import math
    an, ad = alpha
    G = P_min - an * P_min // ad
    Gs = max(1, int(math.floor(G / 4.0 + 0.5)))
    return G, -(-L // G), P_max + an * P_max // ad, Gs, -(-L // Gs)


def _psola_args(fn, wav, f0, lengths, hop, P):
    _chk(wav, f"{fn}: wav"); _chk(f0, f"{fn}: f0")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise _lib.NsgError(f"{fn}: wav {tuple(wav.shape)} is not (B, L) with B, L >= 1")
    B, L = wav.shape
    if f0.dim() != 2 or f0.shape[0] != B or f0.shape[1] < 1 or f0.device != wav.device:
        raise _lib.NsgError(f"{fn}: f0 {tuple(f0.shape)} on {f0.device} is not ({B}, T >= 1) on {wav.device}")
    P_u, P_min, P_max, alpha = P
    if not (2 <= P_min <= P_max and 0 <= alpha[0] and 1 <= alpha[1] and 2 * alpha[0] <= alpha[1]):
        raise _lib.NsgError(f"{fn}: need 2 <= P_min <= P_max and 0 <= alpha <= 1 / 2, got [{P_min}, {P_max}], {alpha[0]} / {alpha[1]}")
    lens = None if lengths is None else _lengths_on(lengths, f"{fn}: lengths", B, 0, L, wav.device)
    return B, L, f0.shape[1], lens, psola_sizes(L, P_min, P_max, alpha)


def pitch_marks(wav, f0, hop, sample_rate, P_u, P_min, P_max, alpha=(1, 4), lengths=None):
    """Pitch marks (include/nsg.h: nsg_audio_pitch_marks).  wav (B, L) fp32 zero-padded clips, f0 (B, T) fp32 Hz (not > 0:
    unvoiced; frame t at sample t hop); lengths as ops.f0 takes them; alpha = (num, den) -> (marks (B, K_max) int32, -1 past a
    clip's marks; n_marks (B,) int32), K_max = psola_sizes(...)[1].  The envelope is the entry point's to state and refuse."""
    B, L, T, lens, (_, K_max, _, _, _) = _psola_args("pitch_marks", wav, f0, lengths, hop, (P_u, P_min, P_max, alpha))
    marks = torch.empty(B, K_max, dtype=torch.int32, device=wav.device)
    n_marks = torch.empty(B, dtype=torch.int32, device=wav.device)
    _lib.call("nsg_audio_pitch_marks", _p(wav), _p(lens), _p(f0), _p(marks), _p(n_marks), B, L, T, int(hop), float(sample_rate), int(P_u), int(P_min),
              int(P_max), int(alpha[0]), int(alpha[1]), K_max, _stream())
    return marks, n_marks


def psola(wav, f0, f0_out, marks, n_marks, hop, sample_rate, P_u, P_min, P_max, alpha=(1, 4), lengths=None):
    """Pitch-synchronous overlap-add (include/nsg.h: nsg_audio_psola).  wav, f0, lengths and the constants as ops.pitch_marks took
    them, marks and n_marks as it returned them, f0_out (B, T) fp32 Hz: the track the output is to have -> (out (B, L) fp32, zeros
    past each clip; syn (B, J_max) int32: the synthesis marks, map (B, J_max) int32: the mark each takes its grain from, both -1
    past a clip's n_syn (B,) int32), J_max = psola_sizes(...)[4]."""
    B, L, T, lens, (_, K_max, _, _, J_max) = _psola_args("psola", wav, f0, lengths, hop, (P_u, P_min, P_max, alpha))
    _chk(f0_out, "psola: f0_out"); _chk(marks, "psola: marks", torch.int32); _chk(n_marks, "psola: n_marks", torch.int32)
    if f0_out.shape != f0.shape or tuple(marks.shape) != (B, K_max) or tuple(n_marks.shape) != (B,) or len({t.device for t in (wav, f0_out, marks, n_marks)}) != 1:
        raise _lib.NsgError(f"psola: f0_out {tuple(f0_out.shape)} / marks {tuple(marks.shape)} / n_marks {tuple(n_marks.shape)} do not go with f0 "
                            f"{tuple(f0.shape)} and K_max = {K_max} on {wav.device}")
    out = torch.empty(B, L, dtype=torch.float32, device=wav.device)
    syn, mp = (torch.empty(B, J_max, dtype=torch.int32, device=wav.device) for _ in range(2))
    n_syn = torch.empty(B, dtype=torch.int32, device=wav.device)
    _lib.call("nsg_audio_psola", _p(wav), _p(lens), _p(f0), _p(f0_out), _p(marks), _p(n_marks), _p(syn), _p(mp), _p(n_syn), _p(out), B, L, T, int(hop),
              float(sample_rate), int(P_u), int(P_min), int(P_max), int(alpha[0]), int(alpha[1]), K_max, J_max, _stream())
    return out, syn, mp, n_syn


def mix_noise(wav, noise, gain, level, offset, lengths=None, out=None, want_energy=False):
    """Gain and noise at a level relative to each clip's RMS (include/nsg.h: nsg_audio_mix_noise).  wav (B, L) fp32 zero-padded
    clips, noise (Ln,) fp32 on the same device (one recording, read cyclically from offset[b]); gain, level: B numbers on the
    host (rounded to fp32); offset: B integers in [0, Ln) on the host (checked here) -- or all three as (B,) fp32 / fp32 / int32
    tensors already on the device, the caller's to have checked; lengths as ops.f0 takes them -> out (B, L) fp32,
        out[b, i] = fl(fl(gain[b] x[b, i]) + fl(s_b noise[(offset[b] + i) mod Ln])),  s_b = (float)(level[b] sqrt(E_x / E_n)),
    +0.0 past a clip's length; with want_energy also (B, 2) fp64 (E_x, E_n), the fp64 sums of squares s_b was formed from."""
    import numpy as np
    _chk(wav, "mix_noise: wav"); _chk(noise, "mix_noise: noise")
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1 or noise.dim() != 1 or noise.shape[0] < 1 or noise.device != wav.device:
        raise _lib.NsgError(f"mix_noise: wav {tuple(wav.shape)} / noise {tuple(noise.shape)} are not (B, L) / (Ln,) on one device, B, L, Ln >= 1")
    B, L = wav.shape
    Ln = noise.shape[0]
    on_device = [isinstance(v, torch.Tensor) and v.is_cuda for v in (gain, level, offset)]
    if all(on_device):                                  # the caller's to have checked on the host copy they came from (the kernel clamps offset)
        for name, v, dtype in (("gain", gain, torch.float32), ("level", level, torch.float32), ("offset", offset, torch.int32)):
            if _chk(v, f"mix_noise: {name}", dtype).shape != (B,) or v.device != wav.device:
                raise _lib.NsgError(f"mix_noise: {name} on the device must be a ({B},) tensor on wav's device, got {tuple(v.shape)}")
        g_d, l_d, o_d = gain, level, offset
    elif any(on_device):
        raise _lib.NsgError("mix_noise: gain, level and offset must be all on the host or all on the device")
    else:
        packed = np.empty((3, B), dtype=np.int32)       # one upload for the three
        for row, (name, v) in enumerate((("gain", gain), ("level", level))):
            a = np.asarray(v, dtype=np.float64)
            a = np.broadcast_to(a, (B,)) if a.ndim == 0 else a
            if a.shape != (B,) or not np.isfinite(a).all():
                raise _lib.NsgError(f"mix_noise: {name} must be {B} finite number(s), got {v!r}")
            packed[row] = a.astype(np.float32).view(np.int32)
        off = np.asarray(offset)
        off = np.broadcast_to(off, (B,)) if off.ndim == 0 else off
        if off.shape != (B,) or not np.issubdtype(off.dtype, np.integer) or off.min() < 0 or off.max() >= Ln:
            raise _lib.NsgError(f"mix_noise: offset must be {B} integer(s) in [0, {Ln}), got {offset!r}")
        packed[2] = off
        packed = torch.from_numpy(packed).to(wav.device)
        g_d, l_d, o_d = packed[0].view(torch.float32), packed[1].view(torch.float32), packed[2]
    lens = None if lengths is None else _lengths_on(lengths, "mix_noise: lengths", B, 0, L, wav.device)
    if out is None:
        out = torch.empty_like(wav)
    elif _chk(out, "mix_noise: out").numel() != B * L or out.device != wav.device or out.data_ptr() == wav.data_ptr():
        raise _lib.NsgError(f"mix_noise: out {tuple(out.shape)} does not hold {B} x {L}, or is wav itself")
    energy = torch.empty(B, 2, dtype=torch.float64, device=wav.device) if want_energy else None
    ws, nb = _ws(wav.device, "nsg_audio_mix_noise_workspace_bytes", B, L)
    _lib.call("nsg_audio_mix_noise", _p(wav), _p(lens), _p(noise), _p(g_d), _p(l_d), _p(o_d), _p(out), _p(energy), B, L, Ln, _p(ws), nb, _stream())
    return (out, energy) if want_energy else out


def vq_ema_update(codebook, ema_n, ema_s, n, s, decay=0.99, eps=1e-5):
    K, D = codebook.shape
    scratch = torch.empty(1, dtype=torch.float32, device=codebook.device)
    _lib.call("nsg_vq_ema_update", _p(codebook), _p(ema_n), _p(ema_s), _p(n), _p(s), K, D, decay, eps, _p(scratch), _stream())


def debug_dot(x, e, mode):
    out = torch.empty(x.shape[0], e.shape[0], dtype=torch.float32, device=x.device)
    _lib.call("nsg_debug_dot", _p(x), _p(e), x.shape[0], x.shape[1], e.shape[0], mode, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------
def conv_desc(B, IH, IW, C_in, C_out, k, stride, pad, transposed=False, dtype=torch.float32, out_hw=None) -> ConvDesc:
    """dtype: storage type of the layer's multi-channel activations and packed weights.  k and pad may be (rows, columns)
    pairs (a rectangular stride-1 Conv2d); out_hw crops a stride-1 output at the bottom / right."""
    kh, kw = (k if isinstance(k, (tuple, list)) else (k, k))
    ph, pw = (pad if isinstance(pad, (tuple, list)) else (pad, pad))
    if transposed:
        OH, OW = (IH - 1) * stride - 2 * ph + kh, (IW - 1) * stride - 2 * pw + kw
    else:
        OH, OW = (IH + 2 * ph - kh) // stride + 1, (IW + 2 * pw - kw) // stride + 1
    if out_hw is not None:
        OH, OW = out_hw
    rect = (kh != kw) or (ph != pw)
    return ConvDesc(B, IH, IW, C_in, OH, OW, C_out, kh, stride, ph, 1 if transposed else 0, nsg_dtype(dtype), kw if rect else 0, pw if rect else 0)


def _in_dtype(d: ConvDesc):
    """torch dtype of the layer INPUT tensor (single-channel images are always fp32)."""
    return torch.float32 if d.C_in == 1 else torch_dtype(d.dtype)


def _out_dtype(d: ConvDesc, flags=0):
    return torch.float32 if (d.C_out == 1 or (flags & NSG_OUT_F32)) else torch_dtype(d.dtype)


def pack_weights(d: ConvDesc, w, want_fwd=True, want_dgrad=True):
    _chk(w, "weight")
    n = _lib.query("nsg_packed_weight_floats", byref(d))
    wf = torch.empty(n, dtype=torch_dtype(d.dtype), device=w.device) if want_fwd else None
    wd = torch.empty(n, dtype=torch_dtype(d.dtype), device=w.device) if want_dgrad else None
    _lib.call("nsg_pack_conv_weights", byref(d), _p(w), _p(wf), _p(wd), _stream())
    return wf, wd


def pack_weights_batch(jobs):
    """jobs: list of (desc, weight, want_fwd, want_dgrad) -> list of (w_fwd, w_dgrad); ONE kernel launch for all of them
    (a training step re-packs every layer's weights after each optimiser step)."""
    n = len(jobs)
    if n == 0:
        return []
    descs = (ConvDesc * n)()
    wp, fp, dp = (c_void_p * n)(), (c_void_p * n)(), (c_void_p * n)()
    out = []
    for i, (d, w, want_fwd, want_dgrad) in enumerate(jobs):
        _chk(w, "weight")
        ne = _lib.query("nsg_packed_weight_floats", byref(d))
        wf = torch.empty(ne, dtype=torch_dtype(d.dtype), device=w.device) if want_fwd else None
        wd = torch.empty(ne, dtype=torch_dtype(d.dtype), device=w.device) if want_dgrad else None
        ctypes.memmove(ctypes.addressof(descs[i]), ctypes.addressof(d), ctypes.sizeof(ConvDesc))
        wp[i] = w.data_ptr()
        fp[i] = wf.data_ptr() if wf is not None else None
        dp[i] = wd.data_ptr() if wd is not None else None
        out.append((wf, wd))
    _lib.tag("pack_weights_batch", 0, sum(4.0 * j[1].numel() for j in jobs) + sum((a.numel() * _es(a) if a is not None else 0) + (b.numel() * _es(b) if b is not None else 0) for a, b in out))
    _lib.call("nsg_pack_conv_weights_batch", n, descs, ctypes.cast(wp, c_void_p), ctypes.cast(fp, c_void_p), ctypes.cast(dp, c_void_p), _stream())
    return out


def _gemm_call(d: ConvDesc, role, name, *args):
    """One forward / dgrad launch of layer d: the census tag, and KERNEL_TIMER's events around the multi-channel layers (the
    single-kernel gather GEMMs) when bench.py has set one."""
    timed = KERNEL_TIMER is not None and d.C_in > 1 and d.C_out > 1
    t0 = KERNEL_TIMER.begin() if timed else None
    _lib.tag(_conv_label(d, role), _gemm_flops(d))
    _lib.call(name, *args)
    if timed:
        KERNEL_TIMER.end("gather_gemm_f32", t0, _gemm_flops(d))


def conv_forward(d: ConvDesc, x, w_fwd, bias, flags=0, out=None):
    """x NHWC (B,IH,IW,C_in) -> y NHWC (B,OH,OW,C_out)."""
    _chk(x, "x", _in_dtype(d))
    if tuple(x.shape) != (d.B, d.IH, d.IW, d.C_in):
        raise _lib.NsgError(f"conv_forward: input shape {tuple(x.shape)} does not match descriptor {d.key()}")
    y = out if out is not None else torch.empty(d.B, d.OH, d.OW, d.C_out, dtype=_out_dtype(d, flags), device=x.device)
    ws, nb = _ws(x.device, "nsg_conv_workspace_bytes", byref(d))
    _gemm_call(d, "forward", "nsg_conv_forward", byref(d), _p(x), _p(w_fwd), _p(bias), _p(y), flags, _p(ws), nb, _stream())
    return y


def conv_forward_bnstats(d: ConvDesc, x, w_fwd, bias, flags=0, running_mean=None, running_var=None, eps=BN_EPS,
                         momentum=BN_MOMENTUM, out=None):
    """conv forward + training-mode BatchNorm statistics of the output in one pass -> (y, mean, invstd)."""
    _chk(x, "x", _in_dtype(d))
    if tuple(x.shape) != (d.B, d.IH, d.IW, d.C_in):
        raise _lib.NsgError(f"conv_forward_bnstats: input shape {tuple(x.shape)} does not match descriptor {d.key()}")
    y = out if out is not None else torch.empty(d.B, d.OH, d.OW, d.C_out, dtype=_out_dtype(d, flags), device=x.device)
    mean = torch.empty(d.C_out, dtype=torch.float32, device=x.device)
    invstd = torch.empty(d.C_out, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_conv_workspace_bytes", byref(d))
    _gemm_call(d, "forward", "nsg_conv_forward_bnstats", byref(d), _p(x), _p(w_fwd), _p(bias), _p(y), flags, eps, momentum, _p(mean), _p(invstd),
               _p(running_mean), _p(running_var), _p(ws), nb, _stream())
    return y, mean, invstd


def conv_dgrad(d: ConvDesc, dy, w_dgrad, out=None, add=None, relu_x=None):
    """dx = conv_dgrad(dy); with add / relu_x: dx = (conv_dgrad(dy) + add) * (relu_x > 0) in the same kernel."""
    _chk(dy, "dy", _out_dtype(d))
    if tuple(dy.shape) != (d.B, d.OH, d.OW, d.C_out):
        raise _lib.NsgError(f"conv_dgrad: dy shape {tuple(dy.shape)} does not match descriptor {d.key()}")
    dx = out if out is not None else torch.empty(d.B, d.IH, d.IW, d.C_in, dtype=_in_dtype(d), device=dy.device)
    ws, nb = _ws(dy.device, "nsg_conv_workspace_bytes", byref(d))
    if add is not None or relu_x is not None:
        for t, nm in ((add, "add"), (relu_x, "relu_x")):
            if t is not None:
                _chk(t, nm, dx.dtype)
                if t.shape != dx.shape:
                    raise _lib.NsgError(f"conv_dgrad: {nm} shape {tuple(t.shape)} does not match dx {tuple(dx.shape)}")
        _gemm_call(d, "dgrad", "nsg_conv_dgrad_relu_add", byref(d), _p(dy), _p(w_dgrad), _p(add), _p(relu_x), _p(dx), 0, _p(ws), nb, _stream())
    else:
        _gemm_call(d, "dgrad", "nsg_conv_dgrad", byref(d), _p(dy), _p(w_dgrad), _p(dx), 0, _p(ws), nb, _stream())
    return dx


def conv_wgrad(d: ConvDesc, x, dy, w_shape, flags=0, dw=None, dbias=None, want_bias=True):
    _chk(x, "x", _in_dtype(d)); _chk(dy, "dy", _out_dtype(d))
    if dw is None:
        dw = torch.empty(w_shape, dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty(d.C_out, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_conv_workspace_bytes", byref(d))
    _lib.tag(_conv_label(d, "wgrad"), _gemm_flops(d))
    _lib.call("nsg_conv_wgrad", byref(d), _p(x), _p(dy), _p(dw), _p(dbias), flags, _p(ws), nb, _stream())
    return dw, dbias


# ------------------------------------------------------------------------------------------------
# batch norm over [M][C]
# ------------------------------------------------------------------------------------------------
def bn_stats(x, C, running_mean=None, running_var=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    _chk(x, "x", None)
    M = x.numel() // C
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_bn_workspace_bytes", M, C)
    _lib.tag("bn_stats", 0, x.numel() * _es(x))
    _lib.call("nsg_bn_stats", _p(x), M, C, nsg_dtype(x.dtype), eps, momentum, _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(ws), nb,
              _stream())
    return mean, invstd


def bn_eval_stats(running_mean, running_var, eps=BN_EPS):
    C = running_mean.numel()
    mean = torch.empty(C, dtype=torch.float32, device=running_mean.device)
    invstd = torch.empty(C, dtype=torch.float32, device=running_mean.device)
    _lib.call("nsg_bn_eval_stats", _p(running_mean), _p(running_var), C, eps, _p(mean), _p(invstd), _stream())
    return mean, invstd


def bn_apply(x, mean, invstd, gamma, beta, relu=False, residual=None, relu_residual=False, out=None, out_dtype=None,
             relu_out=False):
    """out_dtype: storage type of y (default: x's); the residual must have x's type.  relu_out: max(0,.) of the
    final value (the consumer's leading ReLU applied at the producer)."""
    _chk(x, "x", None)
    if residual is not None:
        _chk(residual, "residual", x.dtype)
    C = mean.numel()
    M = x.numel() // C
    y = out if out is not None else torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    _lib.tag("bn_apply", 0, x.numel() * _es(x) * (2 if residual is not None else 1) + y.numel() * _es(y))
    _lib.call("nsg_bn_apply", _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), _p(y), M, C,
              (1 if relu else 0) | (2 if relu_out else 0), 1 if relu_residual else 0, nsg_dtype(x.dtype), nsg_dtype(y.dtype), _stream())
    return y


def bn_backward(x, y_relu, dy, mean, invstd, gamma, dgamma=None, dbeta=None, out=None, dx_colsum=None, relu_beta=None):
    """dx_colsum: optional [C] tensor receiving the column sums of dx (= bias gradient of the conv in front).
    ReLU mask of a fused BatchNorm+ReLU forward: relu_beta (the forward's beta: mask re-derived from x) or
    y_relu (the stored forward output)."""
    _chk(x, "x", None); _chk(dy, "dy", x.dtype)
    if y_relu is not None:
        _chk(y_relu, "y_relu", x.dtype)
    C = mean.numel()
    M = x.numel() // C
    dx = out if out is not None else torch.empty_like(x)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_bn_workspace_bytes", M, C)
    _lib.tag("bn_backward (sums pass + apply pass)", 0, 5.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_backward", _p(x), _p(y_relu), _p(dy), _p(mean), _p(invstd), _p(gamma), _p(relu_beta), _p(dx), _p(dgamma), _p(dbeta),
              _p(dx_colsum), M, C, nsg_dtype(x.dtype), _p(ws), nb, _stream())
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# encoder.0-2 as one operator: Conv2d(1, C, 4, 2, 1) -> BatchNorm2d -> ReLU   (src/models.py:165-167)
# ------------------------------------------------------------------------------------------------
C1_MOMENTS = _lib.NSG_C1_MOMENTS


def c1conv_bn_relu_forward(img, w, bias, gamma, beta, running_mean=None, running_var=None, training=True, eps=1e-5, momentum=0.1,
                           mean=None, invstd=None, out_dtype=torch.float32, moments=None):
    """img fp32 (B, H, W) or (B, H, W, 1); w the Conv2d parameter (C, 1, 4, 4) fp32.  Returns (y NHWC (B, H/2, W/2, C) of
    out_dtype, mean, invstd).  training=False: mean / invstd must be given (bn_eval_stats).  The conv output itself is
    never stored (nsg.h: nsg_c1conv_bn_relu_forward).  moments: optional float64 tensor of C1_MOMENTS elements that receives the
    image's tap moments in training mode (hand it to c1conv_bn_relu_backward: it then skips recomputing them)."""
    _chk(img, "img", torch.float32); _chk(w, "w", torch.float32)
    if moments is not None and (moments.dtype != torch.float64 or moments.numel() != C1_MOMENTS or not moments.is_contiguous()):
        raise ValueError("c1conv_bn_relu_forward: moments must be a contiguous float64 tensor of C1_MOMENTS elements")
    B, H, W = img.shape[0], img.shape[1], img.shape[2]
    C = w.shape[0]
    if w.numel() != C * 16 or img.numel() != B * H * W:
        raise ValueError("c1conv_bn_relu_forward: img must be single-channel and w (C, 1, 4, 4)")
    if training:
        mean = torch.empty(C, dtype=torch.float32, device=img.device)
        invstd = torch.empty(C, dtype=torch.float32, device=img.device)
    elif mean is None or invstd is None:
        raise ValueError("c1conv_bn_relu_forward: eval mode needs mean and invstd")
    y = torch.empty((B, H // 2, W // 2, C), dtype=out_dtype, device=img.device)
    ws, nb = _ws(img.device, "nsg_c1conv_bn_workspace_bytes", C)
    _lib.tag("c1conv_bn_relu_forward (fused input layer)", 2.0 * 16 * y.numel() * (2 if training else 1), 4.0 * img.numel() * (2 if training else 1) + y.numel() * _es(y))
    _lib.call("nsg_c1conv_bn_relu_forward", _p(img), _p(w), _p(bias), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(running_mean), _p(running_var),
              eps, momentum, 1 if training else 0, _p(y), nsg_dtype(out_dtype), B, H, W, C, _p(ws), nb, _p(moments), _stream())
    return y, mean, invstd


def c1conv_bn_relu_backward(img, w, bias, gamma, beta, mean, invstd, dy, dw=None, dbias=None, dgamma=None, dbeta=None, moments=None):
    """Parameter gradients (dw (C, 1, 4, 4), dbias, dgamma, dbeta) of the fused layer from dy (B, H/2, W/2, C).
    moments: what the training forward wrote (same image), or None (recomputed)."""
    _chk(img, "img", torch.float32); _chk(w, "w", torch.float32); _chk(dy, "dy", None)
    B, H, W = img.shape[0], img.shape[1], img.shape[2]
    C = w.shape[0]
    if dy.numel() != B * (H // 2) * (W // 2) * C:
        raise ValueError("c1conv_bn_relu_backward: dy does not match (B, H/2, W/2, C)")
    dev = img.device
    dw = dw if dw is not None else torch.empty_like(w)
    dbias = dbias if dbias is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = dgamma if dgamma is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = dbeta if dbeta is not None else torch.empty(C, dtype=torch.float32, device=dev)
    ws, nb = _ws(dev, "nsg_c1conv_bn_workspace_bytes", C)
    passes = 1.0 if dy.dtype == torch.bfloat16 else 2.0          # bf16: one pass over dy (tap moments), fp32: sums pass + gradient pass
    _lib.tag("c1conv_bn_relu_backward (fused input layer)", 2.0 * 16 * dy.numel() * 3, passes * (4.0 * img.numel() + dy.numel() * _es(dy)))
    _lib.call("nsg_c1conv_bn_relu_backward", _p(img), _p(w), _p(bias), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(dy), nsg_dtype(dy.dtype), _p(dw),
              _p(dbias), _p(dgamma), _p(dbeta), B, H, W, C, _p(ws), nb, _p(moments), _stream())
    return dw, dbias, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# the ResBlock's 1x1 conv with the BatchNorm work around it folded in   (src/models.py:151-155)
# ------------------------------------------------------------------------------------------------
def bn_relu_conv1x1_supported(dtype, C) -> bool:
    return bool(_lib.query("nsg_bn_relu_conv1x1_supported", nsg_dtype(dtype), C))


def bn_relu_conv1x1_forward(x, mean, invstd, gamma, beta, w, bias):
    """y = relu(bn(x)) * w^T + bias on NHWC rows; relu(bn(x)) is never stored.  w (C, C, 1, 1) fp32."""
    _chk(x, "x", None); _chk(w, "w", torch.float32)
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x)
    ws, nb = _ws(x.device, "nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    _lib.tag("flat_gemm 1x1 forward (bn+relu on load)", 2.0 * M * C * C, 2.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_relu_conv1x1_forward", _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(w), _p(bias), _p(y), M, C, nsg_dtype(x.dtype),
              _p(ws), nb, _stream())
    return y


def bn_relu_conv1x1_forward_bnstats(x, mean, invstd, gamma, beta, w, bias, running_mean=None, running_var=None, eps=BN_EPS,
                                    momentum=BN_MOMENTUM):
    """bn_relu_conv1x1_forward plus the batch statistics of its output (for the BatchNorm that follows), taken from the kernel's
    store phase: returns (y, mean_y, invstd_y); running statistics updated in place."""
    _chk(x, "x", None); _chk(w, "w", torch.float32)
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x)
    mean_y = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd_y = torch.empty(C, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    _lib.tag("flat_gemm 1x1 forward (bn+relu on load, stats out)", 2.0 * M * C * C, 2.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_relu_conv1x1_forward_bnstats", _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(w), _p(bias), _p(y), eps, momentum,
              _p(mean_y), _p(invstd_y), _p(running_mean), _p(running_var), M, C, nsg_dtype(x.dtype), _p(ws), nb, _stream())
    return y, mean_y, invstd_y


def bn_relu_conv1x1_wgrad(x, mean, invstd, gamma, beta, dy, dw=None):
    """dw (C, C, 1, 1) = dy^T relu(bn(x)) with the activation rebuilt from x on the operand's way into the MFMA."""
    _chk(x, "x", None); _chk(dy, "dy", x.dtype)
    C = x.shape[-1]
    M = x.numel() // C
    dw = dw if dw is not None else torch.empty((C, C, 1, 1), dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    _lib.tag("wgrad_gemm 1x1 (bn+relu on load)", 2.0 * M * C * C, 2.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_relu_conv1x1_wgrad", _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(dy), _p(dw), M, C, nsg_dtype(x.dtype), _p(ws), nb,
              _stream())
    return dw


def bn_backward_sums(x, dy, mean, invstd, gamma, dgamma=None, dbeta=None, relu_beta=None):
    """The reduction half of bn_backward: (dgamma, dbeta)."""
    _chk(x, "x", None); _chk(dy, "dy", x.dtype)
    C = mean.numel()
    M = x.numel() // C
    dgamma = dgamma if dgamma is not None else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = dbeta if dbeta is not None else torch.empty(C, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_bn_workspace_bytes", M, C)
    _lib.tag("bn_backward_sums", 0, 2.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_backward_sums", _p(x), _p(None), _p(dy), _p(mean), _p(invstd), _p(gamma), _p(relu_beta), _p(dgamma), _p(dbeta), M, C,
              nsg_dtype(x.dtype), _p(ws), nb, _stream())
    return dgamma, dbeta


def bn_backward_conv1x1_dgrad(h, dy, mean, invstd, gamma, dgamma, dbeta, w, dh_colsum=None, prev=None, prev_dgamma=None, prev_dbeta=None):
    """(dh, dx): dh = the BatchNorm's input gradient (no ReLU) at input h, dx = dh * w (the data gradient of the 1x1 conv that
    wrote h); dh_colsum: optional [C] tensor receiving dh's column sums (that conv's bias gradient).
    prev = (prev_x, mean, invstd, gamma, beta) of the BatchNorm + ReLU in front of the conv: its backward sums over (prev_x, dx)
    are formed while dx is written; returns (dh, dx, prev_dgamma, prev_dbeta) then."""
    _chk(h, "h", None); _chk(dy, "dy", h.dtype); _chk(w, "w", torch.float32)
    C = h.shape[-1]
    M = h.numel() // C
    dh, dx = torch.empty_like(h), torch.empty_like(h)
    ws, nb = _ws(h.device, "nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    px = pm = pi = pg = pb = None
    if prev is not None:
        px, pm, pi, pg, pb = prev
        _chk(px, "prev_x", h.dtype)
        prev_dgamma = prev_dgamma if prev_dgamma is not None else torch.empty(C, dtype=torch.float32, device=h.device)
        prev_dbeta = prev_dbeta if prev_dbeta is not None else torch.empty(C, dtype=torch.float32, device=h.device)
    _lib.tag("flat_gemm 1x1 dgrad (bn backward on load)", 2.0 * M * C * C, (5.0 if prev is not None else 4.0) * h.numel() * _es(h))
    _lib.call("nsg_bn_backward_conv1x1_dgrad", _p(h), _p(dy), _p(mean), _p(invstd), _p(gamma), _p(dgamma), _p(dbeta), _p(w), _p(dh), _p(dx),
              _p(dh_colsum), _p(px), _p(pm), _p(pi), _p(pg), _p(pb), _p(prev_dgamma if prev is not None else None),
              _p(prev_dbeta if prev is not None else None), M, C, nsg_dtype(h.dtype), _p(ws), nb, _stream())
    if prev is not None:
        return dh, dx, prev_dgamma, prev_dbeta
    return dh, dx


def bn_backward_conv1x1_dgrad_wgrad_supported(dtype, C) -> bool:
    return bool(_lib.query("nsg_bn_backward_conv1x1_dgrad_wgrad_supported", nsg_dtype(dtype), C))


def bn_backward_conv1x1_dgrad_wgrad(h, dy, mean, invstd, gamma, dgamma, dbeta, w, prev, dh_colsum=None, dw=None, prev_dgamma=None,
                                    prev_dbeta=None):
    """bn_backward_conv1x1_dgrad(..., prev=...) and bn_relu_conv1x1_wgrad in one pass over the tensors: returns
    (dx, dw, prev_dgamma, prev_dbeta); dh is not stored (include/nsg.h: nsg_bn_backward_conv1x1_dgrad_wgrad)."""
    _chk(h, "h", None); _chk(dy, "dy", h.dtype); _chk(w, "w", torch.float32)
    C = h.shape[-1]
    M = h.numel() // C
    px, pm, pi, pg, pb = prev
    _chk(px, "prev_x", h.dtype)
    dev = h.device
    dx = torch.empty_like(h)
    dw = dw if dw is not None else torch.empty_like(w)
    prev_dgamma = prev_dgamma if prev_dgamma is not None else torch.empty(C, dtype=torch.float32, device=dev)
    prev_dbeta = prev_dbeta if prev_dbeta is not None else torch.empty(C, dtype=torch.float32, device=dev)
    ws, nb = _ws(dev, "nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes", M, C)
    _lib.tag("flat_gemm 1x1 dgrad + wgrad (bn backward on load)", 4.0 * M * C * C, 4.0 * h.numel() * _es(h))
    _lib.call("nsg_bn_backward_conv1x1_dgrad_wgrad", _p(h), _p(dy), _p(mean), _p(invstd), _p(gamma), _p(dgamma), _p(dbeta), _p(w), _p(dx), _p(dw),
              _p(dh_colsum), _p(px), _p(pm), _p(pi), _p(pg), _p(pb), _p(prev_dgamma), _p(prev_dbeta), M, C, nsg_dtype(h.dtype), _p(ws), nb, _stream())
    return dx, dw, prev_dgamma, prev_dbeta


def bn_backward_apply(x, dy, mean, invstd, gamma, dgamma, dbeta, relu_beta=None, dx_colsum=None):
    """The apply half of bn_backward with dgamma / dbeta given: dx."""
    _chk(x, "x", None); _chk(dy, "dy", x.dtype)
    C = mean.numel()
    M = x.numel() // C
    dx = torch.empty_like(x)
    ws, nb = _ws(x.device, "nsg_bn_workspace_bytes", M, C)
    _lib.tag("bn_backward_apply", 0, 3.0 * x.numel() * _es(x))
    _lib.call("nsg_bn_backward_apply", _p(x), _p(None), _p(dy), _p(mean), _p(invstd), _p(gamma), _p(relu_beta), _p(dgamma), _p(dbeta), _p(dx),
              _p(dx_colsum), M, C, nsg_dtype(x.dtype), _p(ws), nb, _stream())
    return dx


# ------------------------------------------------------------------------------------------------
# the VAE's Gaussian latent: closing BatchNorm2d(2Z) -> chunk -> KL -> mu + sigma * eps   (src/models.py:77,103-112)
# ------------------------------------------------------------------------------------------------
def _latent_extents(fn, h, eps, dz=None):
    _chk(h, "h"); _chk(eps, "eps")
    C = h.shape[-1]
    M = h.numel() // C
    if C % 2 or eps.numel() != M * (C // 2) or (dz is not None and dz.numel() != eps.numel()):
        raise _lib.NsgError(f"{fn}: h {tuple(h.shape)} holds [M][2Z] rows; eps / dz must hold [M][Z]")
    return M, C // 2


def vae_latent_forward(h, mean, invstd, gamma, beta, eps, z=None, kl=None):
    """h: the closing BatchNorm's INPUT, rows [M][2Z] (mu | logvar after the affine map, formed on load); eps [M][Z].
    Returns (z [M][Z] shaped like eps, kl [1]).  include/nsg.h: nsg_vae_latent_forward."""
    M, Z = _latent_extents("vae_latent_forward", h, eps)
    z = z if z is not None else torch.empty_like(eps)
    kl = kl if kl is not None else torch.empty(1, dtype=torch.float32, device=h.device)
    ws, nb = _ws(h.device, "nsg_vae_latent_workspace_bytes", M, Z)
    _lib.tag("vae_latent_forward", 0, 4.0 * (h.numel() + 2 * eps.numel()))
    _lib.call("nsg_vae_latent_forward", _p(h), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(eps), _p(z), _p(kl), M, Z, _p(ws), nb, _stream())
    return z, kl


def vae_latent_backward(h, mean, invstd, gamma, beta, eps, dz, kl_scale=1.0, kl_grad=None, dy=None, dgamma=None, dbeta=None):
    """(dy [M][2Z] = the gradient at the BatchNorm's output, dgamma, dbeta [2Z] = that BatchNorm's backward sums over dy):
    bn_backward_apply(h, dy, ..., dgamma, dbeta) finishes dh.  kl_grad: one device float (the gradient arriving at kl) or None."""
    M, Z = _latent_extents("vae_latent_backward", h, eps, _chk(dz, "dz"))
    dev = h.device
    dy = dy if dy is not None else torch.empty_like(h)
    dgamma = dgamma if dgamma is not None else torch.empty(2 * Z, dtype=torch.float32, device=dev)
    dbeta = dbeta if dbeta is not None else torch.empty(2 * Z, dtype=torch.float32, device=dev)
    ws, nb = _ws(dev, "nsg_vae_latent_workspace_bytes", M, Z)
    _lib.tag("vae_latent_backward", 0, 4.0 * (2 * h.numel() + 2 * eps.numel()))
    _lib.call("nsg_vae_latent_backward", _p(h), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(eps), _p(dz), float(kl_scale), _p(kl_grad), _p(dy),
              _p(dgamma), _p(dbeta), M, Z, _p(ws), nb, _stream())
    return dy, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# decoder.4-7 as one operator: BatchNorm2d -> ReLU -> ConvTranspose2d(C, 1, 4, 2, 1) [-> Tanh]   (src/models.py:180-183)
# ------------------------------------------------------------------------------------------------
def bn_relu_c1convt_supported(dtype, C) -> bool:
    return bool(_lib.query("nsg_bn_relu_c1convt_supported", nsg_dtype(dtype), C))


def bn_relu_c1convt_forward(u, mean, invstd, gamma, beta, w, bias, tanh=True):
    """u NHWC (B, H, W, C) = the BatchNorm input; w the ConvTranspose2d parameter (C, 1, 4, 4) fp32.  Returns the fp32 image
    (B, 2H, 2W, 1).  relu(bn(u)) is never stored (nsg.h: nsg_bn_relu_c1convt_forward)."""
    _chk(u, "u", None); _chk(w, "w", torch.float32)
    B, H, W, C = u.shape
    y = torch.empty((B, 2 * H, 2 * W, 1), dtype=torch.float32, device=u.device)
    ws, nb = _ws(u.device, "nsg_bn_relu_c1convt_workspace_bytes", B, H, W, C)
    _lib.tag("bn_relu_c1convt_forward (fused output layer)", 2.0 * 16 * u.numel(), u.numel() * _es(u) + 4.0 * y.numel())
    _lib.call("nsg_bn_relu_c1convt_forward", _p(u), nsg_dtype(u.dtype), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(w), _p(bias), _p(y),
              NSG_TANH_OUT if tanh else 0, B, H, W, C, _p(ws), nb, _stream())
    return y


def bn_relu_c1convt_forward_mse(u, mean, invstd, gamma, beta, w, bias, target, grad_scale=1.0, want_image=False, dbias=None):
    """bn_relu_c1convt_forward(tanh=True) + mse_padded + tanh_backward in one pass over the tap products: target fp32
    (B, 2H, T[, 1]) with T >= 2W.  Returns (loss (1,), dpre (B, 2H, 2W, 1) = the gradient w.r.t. the Tanh's input, x_tilde or None).
    dbias: optional (1,) tensor receiving sum(dpre), the transposed conv's bias gradient."""
    _chk(u, "u", None); _chk(w, "w", torch.float32); _chk(target, "target", torch.float32)
    B, H, W, C = u.shape
    T = target.numel() // (B * 2 * H)
    if target.numel() != B * 2 * H * T or T < 2 * W:
        raise ValueError("bn_relu_c1convt_forward_mse: target must be (B, 2H, T) with T >= 2W")
    dev = u.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dpre = torch.empty((B, 2 * H, 2 * W, 1), dtype=torch.float32, device=dev)
    y = torch.empty((B, 2 * H, 2 * W, 1), dtype=torch.float32, device=dev) if want_image else None
    ws, nb = _ws(dev, "nsg_bn_relu_c1convt_workspace_bytes", B, H, W, C)
    _lib.tag("bn_relu_c1convt_forward_mse (fused output layer + loss)", 2.0 * 16 * u.numel(),
             u.numel() * _es(u) + 4.0 * (2 * dpre.numel() + (dpre.numel() if want_image else 0)))
    _lib.call("nsg_bn_relu_c1convt_forward_mse", _p(u), nsg_dtype(u.dtype), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(w), _p(bias), _p(y),
              _p(target), T, grad_scale, _p(loss), _p(dpre), _p(dbias), B, H, W, C, _p(ws), nb, _stream())
    return loss, dpre, y


def bn_relu_c1convt_backward(u, mean, invstd, gamma, beta, w, dy, dw=None, dbias=None, dgamma=None, dbeta=None, du_colsum=None,
                             want_dbias=True):
    """dy: fp32 gradient image (B, 2H, 2W[, 1]) w.r.t. the transposed conv's output (before the tanh).
    Returns (du like u, dw (C, 1, 4, 4), dbias (1,), dgamma, dbeta); du_colsum: optional [C] tensor receiving the column
    sums of du (the bias gradient of the conv in front of the BatchNorm).  want_dbias=False: the bias gradient (sum of dy) is
    not formed (bn_relu_c1convt_forward_mse already gave it); dbias is returned as passed."""
    _chk(u, "u", None); _chk(w, "w", torch.float32); _chk(dy, "dy", torch.float32)
    B, H, W, C = u.shape
    if dy.numel() != B * 4 * H * W:
        raise ValueError("bn_relu_c1convt_backward: dy does not match (B, 2H, 2W)")
    dev = u.device
    du = torch.empty_like(u)
    dw = dw if dw is not None else torch.empty_like(w)
    if want_dbias:
        dbias = dbias if dbias is not None else torch.empty(1, dtype=torch.float32, device=dev)
    dgamma = dgamma if dgamma is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = dbeta if dbeta is not None else torch.empty(C, dtype=torch.float32, device=dev)
    ws, nb = _ws(dev, "nsg_bn_relu_c1convt_workspace_bytes", B, H, W, C)
    _lib.tag("bn_relu_c1convt_backward (fused output layer)", 2.0 * 16 * u.numel() * 3, 3.0 * u.numel() * _es(u) + 2.0 * 4.0 * dy.numel())
    _lib.call("nsg_bn_relu_c1convt_backward", _p(u), nsg_dtype(u.dtype), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(w), _p(dy), _p(du),
              _p(du_colsum), _p(dw), _p(dbias if want_dbias else None), _p(dgamma), _p(dbeta), B, H, W, C, _p(ws), nb, _stream())
    return du, dw, dbias, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# element-wise / losses / optimiser
# ------------------------------------------------------------------------------------------------
def relu_backward_add(a, b, x, out=None):
    _chk(a, "a", x.dtype)
    if b is not None:
        _chk(b, "b", x.dtype)
    dx = out if out is not None else torch.empty_like(x)
    _lib.call("nsg_relu_backward_add", _p(a), _p(b), _p(x), _p(dx), x.numel(), nsg_dtype(x.dtype), _stream())
    return dx


def convert(src, dtype, out=None, relu=False):
    """Change of storage type (fp32 <-> bf16), optionally with max(0,.), by the library's own kernel."""
    _chk(src, "src", None)
    if src.dtype == dtype and out is None and not relu:
        return src
    dst = out if out is not None else torch.empty(src.shape, dtype=dtype, device=src.device)
    _lib.tag("convert", 0, src.numel() * _es(src) + dst.numel() * _es(dst))
    _lib.call("nsg_convert", _p(src), nsg_dtype(src.dtype), _p(dst), nsg_dtype(dst.dtype), src.numel(), 1 if relu else 0, _stream())
    return dst


def tanh_backward(g, y, out=None):
    dx = out if out is not None else torch.empty_like(y)
    _lib.tag("tanh_backward", 0, 12.0 * y.numel())
    _lib.call("nsg_tanh_backward", _p(g), _p(y), _p(dx), y.numel(), _stream())
    return dx


def add(a, b, out=None):
    y = out if out is not None else torch.empty_like(a)
    _lib.call("nsg_add", _p(a), _p(b), _p(y), a.numel(), _stream())
    return y


def add_per_clip(x, rows, out=None, out_dtype=torch.float32):
    """x fp32 NHWC (B,H,W,C) + rows (B,C) broadcast over each clip's pixels -> y of out_dtype."""
    _chk(x, "x"); _chk(rows, "rows")
    B, C = rows.shape
    y = out if out is not None else torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _lib.call("nsg_add_per_clip", _p(x), _p(rows), _p(y), B, x.numel() // (B * C), C, nsg_dtype(y.dtype), _stream())
    return y


def clip_colsum(x, B):
    """x NHWC (B,H,W,C) -> (B,C): per-clip sum over pixels."""
    _chk(x, "x", None)
    C = x.shape[-1]
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    ws, nb = _ws(x.device, "nsg_clip_colsum_workspace_bytes", B, C)
    _lib.call("nsg_clip_colsum", _p(x), nsg_dtype(x.dtype), B, x.numel() // (B * C), C, _p(out), _p(ws), nb, _stream())
    return out


def add_cond(x, table, bins, idx=None, clip_rows=None, relu=False, out=None, out_dtype=torch.float32, grid=None):
    """The F0- (and speaker-) conditioned decoder input in one pass (include/nsg.h: nsg_add_cond):
        y[b, h, w] = act((src[b, h, w] + clip_rows[b]) + table[bins[b, w]])
    x: the fp32 NHWC rows (B, H, W, C) themselves, or -- with idx (B, H, W) int64 -- a (K, C) fp32 table they are gathered from
    (src = x[idx]); table (n_rows, C) fp32; bins (B, W) int64; clip_rows (B, C) fp32 or None; act = ReLU with relu=True.
    -> y (B, H, W, C) of out_dtype.  Out-of-range bins / idx values are clamped by the kernel, never read out of a table.
    grid: (B, H, W) where x's own shape does not say it (rows mode with x given as (N, C))."""
    _chk(x, "add_cond: x"); _chk(table, "add_cond: table"); _chk(bins, "add_cond: bins", torch.int64)
    if table.dim() != 2 or bins.dim() != 2 or x.dim() < 2 or x.shape[-1] != table.shape[1]:
        raise _lib.NsgError(f"add_cond: x {tuple(x.shape)} / table {tuple(table.shape)} / bins {tuple(bins.shape)} are not (.., C) / (n_rows, C) / (B, W)")
    C = table.shape[1]
    B, Wd = bins.shape
    if idx is not None:
        _chk(idx, "add_cond: idx", torch.int64)
        if x.dim() != 2:
            raise _lib.NsgError(f"add_cond: with idx, x {tuple(x.shape)} must be a (K, C) table")
        shape = tuple(idx.shape) if grid is None else tuple(grid)
        K = x.shape[0]
    else:
        shape = tuple(x.shape[:-1]) if grid is None else tuple(grid)
        K = 0
    if len(shape) != 3 or shape[0] != B or shape[2] != Wd or (idx.numel() if idx is not None else x.numel() // C) != B * shape[1] * Wd:
        raise _lib.NsgError(f"add_cond: the latent grid {shape} does not go with bins {tuple(bins.shape)} (B, H, W) / (B, W)")
    H = shape[1]
    if clip_rows is not None and tuple(_chk(clip_rows, "add_cond: clip_rows").shape) != (B, C):
        raise _lib.NsgError(f"add_cond: clip_rows {tuple(clip_rows.shape)} is not ({B}, {C})")
    if len({t.device for t in (x, table, bins, idx, clip_rows) if t is not None}) != 1:
        raise _lib.NsgError("add_cond: the tensors are not on one device")
    if out is None:
        out = torch.empty(B, H, Wd, C, dtype=out_dtype, device=x.device)
    elif _chk(out, "add_cond: out", None).numel() != B * H * Wd * C or out.device != x.device:
        raise _lib.NsgError(f"add_cond: out {tuple(out.shape)} does not hold {B} x {H} x {Wd} x {C}")
    nrow = B * H * Wd
    # (the tables stay in cache: the rows read -- or, gathering, the indices -- and the rows written are what moves)
    _lib.tag("add_cond (gather)" if idx is not None else "add_cond", 0, float(nrow * C * _es(out) + (8 * nrow if idx is not None else 4 * nrow * C)))
    _lib.call("nsg_add_cond", _p(x), _p(idx), _p(clip_rows), _p(table), _p(bins), _p(out), B, H, Wd, C, K, table.shape[0], 1 if relu else 0,
              nsg_dtype(out.dtype), _stream())
    return out


def column_sum(x, out=None):
    """x NHWC (B, H, W, C) fp32 or bf16 -> (B, W, C) fp32: the sum over h, in ascending h in fp32 (include/nsg.h: nsg_column_sum);
    two calls give the same bits."""
    _chk(x, "column_sum: x", None)
    if x.dim() != 4:
        raise _lib.NsgError(f"column_sum: x {tuple(x.shape)} is not (B, H, W, C)")
    B, H, Wd, C = x.shape
    if out is None:
        out = torch.empty(B, Wd, C, dtype=torch.float32, device=x.device)
    elif _chk(out, "column_sum: out").numel() != B * Wd * C or out.device != x.device:
        raise _lib.NsgError(f"column_sum: out {tuple(out.shape)} does not hold {B} x {Wd} x {C}")
    _lib.tag("column_sum", 0, x.numel() * _es(x) + 4.0 * B * Wd * C)
    _lib.call("nsg_column_sum", _p(x), nsg_dtype(x.dtype), B, H, Wd, C, _p(out), _stream())
    return out


def f0_bins(f0, W, n_bins, fmin, fmax, frames=None, affine=None, want_logf=False, out=None):
    """An F0 track at the mel frame rate -> one bin per latent column (include/nsg.h: nsg_f0_bins).  f0 (B, T) fp32 Hz (+0.0:
    unvoiced), T >= 4 W; frames: None (all T), or (B,) frame counts in [0, T] (host: checked here and uploaded; int32 on the
    device: the caller's); affine (B, 3) fp32 rows of (mu_src, ratio, mu_tgt) or None -> bins (B, W) int64: 0 for an unvoiced
    column, 1 .. n_bins otherwise; with want_logf also logf (B, W) fp32, the column's (moved) mean log2 F0, +0.0 where unvoiced.
    out: bins, or (bins, logf), to write instead of new tensors."""
    _chk(f0, "f0_bins: f0")
    if f0.dim() != 2 or f0.shape[0] < 1 or f0.shape[1] < 1:
        raise _lib.NsgError(f"f0_bins: f0 {tuple(f0.shape)} is not (B, T) with B, T >= 1")
    B, T = f0.shape
    W = int(W)
    fr = None if frames is None else _lengths_on(frames, "f0_bins: frames", B, 0, T, f0.device)
    if affine is not None and (tuple(_chk(affine, "f0_bins: affine").shape) != (B, 3) or affine.device != f0.device):
        raise _lib.NsgError(f"f0_bins: affine {tuple(affine.shape)} is not ({B}, 3) on f0's device")
    if out is None:
        bins = torch.empty(B, max(W, 0), dtype=torch.int64, device=f0.device)
        logf = torch.empty(B, max(W, 0), dtype=torch.float32, device=f0.device) if want_logf else None
    else:
        bins, logf = out if want_logf else (out, None)
        for t, name, dtype in ((bins, "bins", torch.int64), (logf, "logf", torch.float32)):
            if t is not None and (_chk(t, f"f0_bins: out {name}", dtype).numel() != B * W or t.device != f0.device):
                raise _lib.NsgError(f"f0_bins: out {name} {tuple(t.shape)} does not hold {B} x {W}")
    _lib.call("nsg_f0_bins", _p(f0), _p(fr), _p(affine), _p(bins), _p(logf), B, T, W, int(n_bins), float(fmin), float(fmax), _stream())
    return (bins, logf) if want_logf else bins


def collate_f0_bins(f0_corpus, plan, T, n_bins, fmin, fmax, W=None, affine=None, want_logf=False, want_f0=False):
    """A batch's F0 bins straight from a resident track (include/nsg.h: nsg_collate_f0_bins): f0_corpus (frames,) fp32 Hz (+0.0:
    unvoiced), laid out as the mel corpus' frames are; plan (B, 3) int64 rows of (clip, start, count), collate_mels' own; T the
    batch's width; W latent columns (default T // 4; T >= 4 W).  Exactly f0_bins of the rows collate_mels' rule would crop
    (f0_corpus[start_b : start_b + count_b], +0.0 up to T) with frames = count_b -- one launch, the rows never stored.
    affine (B, 3) fp32 or None, as in f0_bins.  -> bins (B, W) int64; with want_logf / want_f0 the tuple (bins[, logf (B, W) fp32]
    [, f0 (B, T) fp32: the cropped rows]).  A plan on the device is the caller's to have checked (check_collate_plan on its host
    copy); a plan on the host is checked here and uploaded."""
    for t, name, dtype in ((f0_corpus, "f0_corpus", torch.float32), (plan, "plan", torch.int64)):
        if t.dtype != dtype:
            raise _lib.NsgError(f"collate_f0_bins: {name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.NsgError(f"collate_f0_bins: {name}: expected a contiguous tensor")
    if f0_corpus.dim() != 1:
        raise _lib.NsgError(f"collate_f0_bins: f0_corpus {tuple(f0_corpus.shape)} is not (frames,)")
    if plan.dim() != 2 or plan.shape[1] != 3 or plan.shape[0] < 1:
        raise _lib.NsgError(f"collate_f0_bins: plan {tuple(plan.shape)} is not (B, 3) with B >= 1")
    T = int(T)
    W = T // 4 if W is None else int(W)
    frames, B = f0_corpus.shape[0], plan.shape[0]
    if not plan.is_cuda:
        check_collate_plan(plan, T, frames)
    _chk(f0_corpus, "collate_f0_bins: f0_corpus")
    if not plan.is_cuda:
        plan = plan.to(f0_corpus.device)
    dev = f0_corpus.device
    if affine is not None and (tuple(_chk(affine, "collate_f0_bins: affine").shape) != (B, 3) or affine.device != dev):
        raise _lib.NsgError(f"collate_f0_bins: affine {tuple(affine.shape)} is not ({B}, 3) on f0_corpus' device")
    if plan.device != dev:
        raise _lib.NsgError("collate_f0_bins: plan and f0_corpus are not on one device")
    bins = torch.empty(B, max(W, 0), dtype=torch.int64, device=dev)
    logf = torch.empty(B, max(W, 0), dtype=torch.float32, device=dev) if want_logf else None
    f0 = torch.empty(B, max(T, 0), dtype=torch.float32, device=dev) if want_f0 else None
    _lib.call("nsg_collate_f0_bins", _p(f0_corpus), frames, _p(plan), _p(affine), _p(bins), _p(logf), _p(f0), B, T, W, int(n_bins),
              float(fmin), float(fmax), _stream())
    out = (bins,) + ((logf,) if want_logf else ()) + ((f0,) if want_f0 else ())
    return out if len(out) > 1 else bins


def mse_padded(a, c, rows, wa, wc, grad_scale=1.0, want_grad=True):
    """mean((pad(a) - c)^2) with a zero-padded from width wa to wc (train.py:118-129)."""
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    ws, nb = _ws(a.device, "nsg_reduce_workspace_bytes", rows * wc)
    _lib.tag("mse_padded (loss + gradient)", 0, 4.0 * (a.numel() * (2 if want_grad else 1) + c.numel()))
    _lib.call("nsg_mse_padded", _p(a), _p(c), rows, wa, wc, grad_scale, _p(loss), _p(da), _p(ws), nb, _stream())
    return loss, da


def vq_losses(z, q, dz_scale=1.0, dq_scale=1.0, dz_add=None, want_dz=True, want_dq=True, grad_dtype=torch.float32):
    """mean((q - z)^2) and its two one-sided gradients (train.py:131,133).  z, q, dq fp32; dz (and dz_add,
    the straight-through gradient coming out of the decoder) in grad_dtype."""
    _chk(z, "z"); _chk(q, "q")
    if dz_add is not None:
        _chk(dz_add, "dz_add", grad_dtype)
    n = z.numel()
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty(z.shape, dtype=grad_dtype, device=z.device) if want_dz else None
    dq = torch.empty_like(z) if want_dq else None
    ws, nb = _ws(z.device, "nsg_reduce_workspace_bytes", n)
    _lib.tag("vq_losses", 0, 4.0 * n * 2 + (dz.numel() * _es(dz) * (2 if dz_add is not None else 1) if dz is not None else 0) + (4.0 * n if dq is not None else 0))
    _lib.call("nsg_vq_losses", _p(z), _p(q), n, dz_scale, dq_scale, _p(dz_add), _p(loss), _p(dz), _p(dq), nsg_dtype(grad_dtype), _p(ws), nb,
              _stream())
    return loss, dz, dq


def vq_losses_indexed_bn_supported(D) -> bool:
    return bool(_lib.query("nsg_vq_losses_indexed_bn_supported", D))


def vq_losses_indexed(z2d, codebook, idx, dz_scale=1.0, dz_add=None, want_dz=True, grad_dtype=torch.float32, bn=None, dgamma=None,
                      dbeta=None):
    """vq_losses with q = codebook[idx] read from the codebook itself: returns (loss, dz).  z2d (N, D) fp32.
    bn = (x, mean, invstd): dz is the incoming gradient of a BatchNorm with input x (N, D) of grad_dtype; returns
    (loss, dz, dgamma, dbeta) with that BatchNorm's backward sums (= bn_backward_sums(x, dz, ...)) formed while dz is written."""
    _chk(codebook, "codebook"); _chk(idx, "idx", torch.int64)
    if dz_add is not None:
        _chk(dz_add, "dz_add", grad_dtype)
    if isinstance(z2d, BnResRows):
        return _vq_losses_indexed_bnres(z2d.check("vq_losses_indexed"), codebook, idx, dz_scale, dz_add, want_dz, grad_dtype, bn, dgamma, dbeta)
    _chk(z2d, "z")
    N, D = z2d.shape
    loss = torch.empty(1, dtype=torch.float32, device=z2d.device)
    dz = torch.empty(z2d.shape, dtype=grad_dtype, device=z2d.device) if want_dz else None
    if bn is not None:
        x, mean, invstd = bn
        _chk(x, "bn x", grad_dtype); _chk(mean, "bn mean"); _chk(invstd, "bn invstd")
        if dz is None or x.numel() != N * D:
            raise _lib.NsgError("vq_losses_indexed: bn= needs want_dz and a BatchNorm input of z's shape")
        dgamma = dgamma if dgamma is not None else torch.empty(D, dtype=torch.float32, device=z2d.device)
        dbeta = dbeta if dbeta is not None else torch.empty(D, dtype=torch.float32, device=z2d.device)
        ws, nb = _ws(z2d.device, "nsg_vq_losses_indexed_bn_workspace_bytes", N, D)
        _lib.tag("vq_losses_indexed", 0, 4.0 * N * D + 8.0 * N + dz.numel() * _es(dz) * (3 if dz_add is not None else 2))
        _lib.call("nsg_vq_losses_indexed_bn", _p(z2d), _p(codebook), _p(idx), N, D, codebook.shape[0], dz_scale, _p(dz_add), _p(loss), _p(dz),
                  nsg_dtype(grad_dtype), _p(x), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(ws), nb, _stream())
        return loss, dz, dgamma, dbeta
    ws, nb = _ws(z2d.device, "nsg_reduce_workspace_bytes", N * D)
    _lib.tag("vq_losses_indexed", 0, 4.0 * N * D + 8.0 * N + (dz.numel() * _es(dz) * (2 if dz_add is not None else 1) if dz is not None else 0))
    _lib.call("nsg_vq_losses_indexed", _p(z2d), _p(codebook), _p(idx), N, D, codebook.shape[0], dz_scale, _p(dz_add), _p(loss), _p(dz),
              nsg_dtype(grad_dtype), _p(ws), nb, _stream())
    return loss, dz


def _vq_losses_indexed_bnres(z, codebook, idx, dz_scale, dz_add, want_dz, grad_dtype, bn, dgamma, dbeta):
    """vq_losses_indexed on rows given as their sources: they ARE the output of the BatchNorm whose backward sums bn= asks for,
    so bn must be that BatchNorm, (z.h, z.mean, z.invstd); z.h is then read once for both uses.  Returns (loss, dz, dgamma, dbeta)."""
    N, D = z.shape
    if bn is None or not want_dz or grad_dtype != torch.bfloat16 or not bnres_rows_supported(D):
        raise _lib.NsgError("vq_losses_indexed: rows given as their sources need bn=, want_dz, bf16 gradients and D a power of two <= 256")
    if bn[0].data_ptr() != z.h.data_ptr() or bn[1].data_ptr() != z.mean.data_ptr() or bn[2].data_ptr() != z.invstd.data_ptr():
        raise _lib.NsgError("vq_losses_indexed: bn= must be the BatchNorm the rows' sources name (h, mean, invstd)")
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty(z.shape, dtype=grad_dtype, device=z.device)
    dgamma = dgamma if dgamma is not None else torch.empty(D, dtype=torch.float32, device=z.device)
    dbeta = dbeta if dbeta is not None else torch.empty(D, dtype=torch.float32, device=z.device)
    ws, nb = _ws(z.device, "nsg_vq_losses_indexed_bn_workspace_bytes", N, D)
    # h, r and dz_add in, dz out (bf16), the indices; the codebook rows come from cache
    _lib.tag("vq_losses_indexed", 0, 2.0 * N * D * 2 + 8.0 * N + dz.numel() * _es(dz) * (2 if dz_add is not None else 1))
    _lib.call("nsg_vq_losses_indexed_bnres", *z.pointers(), _p(codebook), _p(idx), N, D, codebook.shape[0], dz_scale, _p(dz_add), _p(loss), _p(dz),
              _p(dgamma), _p(dbeta), _p(ws), nb, _stream())
    return loss, dz, dgamma, dbeta


def adam_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _lib.tag("adam_step", 0, 28.0 * p.numel())
    _lib.call("nsg_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _stream())


def grad_sumsq(g, out=None):
    """sum(g^2) of a contiguous fp32 tensor, accumulated in double in a fixed order: a float64 tensor of one element that stays
    on the device (`out` to reuse one).  No host synchronisation."""
    _chk(g, "g")
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    elif out.dtype != torch.float64 or not out.is_cuda or out.numel() != 1:
        raise _lib.NsgError("grad_sumsq: out must be one float64 on the GPU")
    ws, nb = _ws(g.device, "nsg_grad_sumsq_workspace_bytes", g.numel())
    _lib.tag("grad_sumsq", 0, 4.0 * g.numel())
    _lib.call("nsg_grad_sumsq", _p(g), g.numel(), _p(out), _p(ws), nb, _stream())
    return out


def new_adamw_stats(device):
    """The 16-byte statistics block of adamw_step, zeroed: see read_adamw_stats."""
    return torch.zeros(4, dtype=torch.int32, device=device)


def read_adamw_stats(stats):
    """(norm, coef, finite, skipped steps) of a statistics block; synchronises.  norm is -1 when no sum of squares was given."""
    host = stats.cpu()
    f = host.view(torch.float32)
    return float(f[0]), float(f[1]), int(host[2]), int(host[3])


def adamw_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, seg_end=None, seg_wd=None, sumsq=None,
               max_norm=0.0, skip_nonfinite=False, shadow=None, one_minus_decay=0.0, stats=None):
    """adam_step with decoupled weight decay per segment (seg_end int64 / seg_wd fp32 device tables), clipping by the global
    norm (sumsq from grad_sumsq, max_norm > 0), the non-finite guard, a weight EMA into `shadow` and the statistics block
    (new_adamw_stats); every option off gives adam_step's bits."""
    S = 0
    if seg_end is not None or seg_wd is not None:
        if seg_end is None or seg_wd is None:
            raise _lib.NsgError("adamw_step: seg_end and seg_wd come together")
        _chk(seg_end, "seg_end", torch.int64); _chk(seg_wd, "seg_wd", torch.float32)
        S = seg_end.numel()
        if seg_wd.numel() != S:
            raise _lib.NsgError("adamw_step: seg_end and seg_wd differ in length")
    if sumsq is not None:
        _chk(sumsq, "sumsq", torch.float64)
    if shadow is not None:
        _chk(shadow, "shadow", torch.float32)
        if shadow.numel() != p.numel():
            raise _lib.NsgError("adamw_step: shadow and p differ in length")
    if stats is not None and (not stats.is_cuda or stats.numel() * stats.element_size() < 16):
        raise _lib.NsgError("adamw_step: stats must be 16 bytes on the GPU")
    n = p.numel()
    _lib.tag("adamw_step", 0, (28.0 + (8.0 if shadow is not None else 0.0)) * n)
    _lib.call("nsg_adamw_step", _p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, step, grad_scale, _p(seg_end), _p(seg_wd), S,
              _p(sumsq), float(max_norm), 1 if skip_nonfinite else 0, _p(shadow), float(one_minus_decay), _p(stats), _stream())


# ------------------------------------------------------------------------------------------------
# latent prior (GatedPixelCNN): element-wise pieces
# ------------------------------------------------------------------------------------------------
def gated_activation(x, cond=None, out=None):
    """x (..., 2C) NHWC rows, cond (B, 2C) or None -> tanh(a) * sigmoid(b) of the channel halves, (..., C)."""
    _chk(x, "x")
    C2 = x.shape[-1]
    M = x.numel() // C2
    y = _gate_out(out, x.shape[:-1] + (C2 // 2,), x.device, "gated_activation: out")
    rpc = 1
    if cond is not None:
        _chk(cond, "cond")
        if cond.shape[-1] != C2 or M % cond.shape[0] != 0:
            raise _lib.NsgError(f"gated_activation: cond {tuple(cond.shape)} does not match x {tuple(x.shape)}")
        rpc = M // cond.shape[0]
    _lib.call("nsg_gated_activation_forward", _p(x), _p(cond), _p(y), M, C2 // 2, rpc, _stream())
    return y


def gated_activation_backward(x, cond, dy):
    _chk(x, "x"); _chk(dy, "dy")
    C2 = x.shape[-1]
    M = x.numel() // C2
    dx = torch.empty_like(x)
    rpc = M // cond.shape[0] if cond is not None else 1
    _lib.call("nsg_gated_activation_backward", _p(x), _p(cond), _p(dy), _p(dx), M, C2 // 2, rpc, _stream())
    return dx


def _gate_out(out, shape, device, name):
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if tuple(_chk(out, name).shape) != tuple(shape):
        raise _lib.NsgError(f"{name} has shape {tuple(out.shape)}, expected {tuple(shape)}")
    return out


def _gate_extents(fn, x, cond, dy=None, x2=None, n_clips=None):
    """Checks shared by the gate wrappers -> (M, C, rows_per_clip, B); B from cond, else n_clips, else None."""
    _chk(x, "x")
    C2 = x.shape[-1]
    M = x.numel() // C2
    if x2 is not None and _chk(x2, "b").shape != x.shape:
        raise _lib.NsgError(f"{fn}: the summands {tuple(x.shape)} and {tuple(x2.shape)} differ in shape")
    if dy is not None and (_chk(dy, "dy").numel() != M * (C2 // 2) or dy.shape[-1] != C2 // 2):
        raise _lib.NsgError(f"{fn}: dy {tuple(dy.shape)} does not match x {tuple(x.shape)}")
    B = None
    if cond is not None:
        _chk(cond, "cond")
        if cond.dim() != 2 or cond.shape[-1] != C2 or M % cond.shape[0] != 0:
            raise _lib.NsgError(f"{fn}: cond {tuple(cond.shape)} does not match x {tuple(x.shape)}")
        B = cond.shape[0]
    if n_clips is not None:
        if (B is not None and B != n_clips) or n_clips < 1 or M % n_clips != 0:
            raise _lib.NsgError(f"{fn}: {n_clips} clips do not match x {tuple(x.shape)} / cond")
        B = n_clips
    return M, C2 // 2, (M // B if B else 1), B


def gated_activation_sum(a, b, cond=None, out=None):
    """gate((a + b) + cond) of two summands (..., 2C): what gated_activation(add(a, b), cond) returns, bit for bit, without the
    sum in memory (nsg_gated_activation_sum_forward)."""
    M, C, rpc, _ = _gate_extents("gated_activation_sum", a, cond, x2=b)
    y = _gate_out(out, a.shape[:-1] + (C,), a.device, "gated_activation_sum: out")
    _lib.tag("gated_activation_sum", 0, 4.0 * M * C * 5)
    _lib.call("nsg_gated_activation_sum_forward", _p(a), _p(b), _p(cond), _p(y), M, C, rpc, _stream())
    return y


def _gate_backward(fn, entry, x, x2, cond, dy, out, dcond, want_dcond, n_clips):
    M, C, rpc, B = _gate_extents(fn, x, cond, dy=dy, x2=x2, n_clips=n_clips)
    dx = _gate_out(out, x.shape, x.device, fn + ": out")
    ws, nb = None, 0
    if want_dcond or dcond is not None:
        if B is None:
            raise _lib.NsgError(f"{fn}: the column sums need cond or n_clips")
        dcond = _gate_out(dcond, (B, 2 * C), x.device, fn + ": dcond")
        ws, nb = _ws(x.device, "nsg_gated_colsum_workspace_bytes", M, C, rpc)
        if nb == 0:
            raise _lib.NsgError(f"{fn}: the column sums take C % 4 == 0, C <= 1024 (C = {C})")
    _lib.tag(fn, 0, 4.0 * M * C * (5 + (2 if x2 is not None else 0)))
    head = (_p(x), _p(x2)) if x2 is not None else (_p(x),)
    _lib.call(entry, *head, _p(cond), _p(dy), _p(dx), _p(dcond), M, C, rpc, _p(ws), nb, _stream())
    return dx, dcond


def gated_activation_sum_backward(a, b, cond, dy, out=None, dcond=None, want_dcond=False, n_clips=None):
    """Backward of gated_activation_sum -> (dx, dcond): dx (..., 2C) is the gradient of both summands; dcond (B, 2C), the
    per-clip column sums of dx, when want_dcond or a dcond buffer is given (else None).  n_clips: B when there is no cond."""
    return _gate_backward("gated_activation_sum_backward", "nsg_gated_activation_sum_backward", a, b, cond, dy, out, dcond, want_dcond, n_clips)


def gated_activation_backward_colsum(x, cond, dy, out=None, dcond=None, n_clips=None):
    """gated_activation_backward with the per-clip column sums of dx formed in the same pass -> (dx, dcond (B, 2C))."""
    return _gate_backward("gated_activation_backward_colsum", "nsg_gated_activation_backward_colsum", x, None, cond, dy, out, dcond, True, n_clips)


def cross_entropy(logits2d, target, want_grad=True, grad_scale=1.0):
    """mean cross-entropy of rows (M, K) against int64 targets (M,) -> (loss[1], dlogits or None)."""
    _chk(logits2d, "logits"); _chk(target, "target", torch.int64)
    M, K = logits2d.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits2d.device)
    dl = torch.empty_like(logits2d) if want_grad else None
    ws, nb = _ws(logits2d.device, "nsg_cross_entropy_workspace_bytes", M)
    _lib.call("nsg_cross_entropy", _p(logits2d), _p(target), M, K, grad_scale, _p(loss), _p(dl), _p(ws), nb, _stream())
    return loss, dl


def cross_entropy_masked(logits2d, target, rows_per_clip, want_grad=True, grad_scale=1.0, want_clip=False, out=None):
    """Mean cross-entropy over the rows whose target is >= 0 (nsg_cross_entropy_masked): rows (M, K), int64 targets (M,),
    M = B * rows_per_clip -> (loss[1], dlogits or None, clip_nll (B,) fp32 or None, clip_count (B,) int64 or None).  Nothing
    valid: loss 0, zero gradient.  out: optional (M, K) destination of the gradient."""
    _chk(logits2d, "logits"); _chk(target, "target", torch.int64)
    M, K = logits2d.shape
    rows_per_clip = int(rows_per_clip)
    if target.numel() != M or rows_per_clip < 1 or M % rows_per_clip != 0:
        raise _lib.NsgError(f"cross_entropy_masked: {M} rows, {target.numel()} targets, clips of {rows_per_clip} rows")
    B = M // rows_per_clip
    dev = logits2d.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dl = _gate_out(out, (M, K), dev, "cross_entropy_masked: out") if (want_grad or out is not None) else None
    nll = torch.empty(B, dtype=torch.float32, device=dev) if want_clip else None
    cnt = torch.empty(B, dtype=torch.int64, device=dev) if want_clip else None
    ws, nb = _ws(dev, "nsg_cross_entropy_masked_workspace_bytes", M, rows_per_clip)
    _lib.tag("cross_entropy_masked", 0, 4.0 * M * K * (2 if dl is not None else 1))
    _lib.call("nsg_cross_entropy_masked", _p(logits2d), _p(target), M, K, rows_per_clip, grad_scale, _p(loss), _p(dl), _p(nll), _p(cnt), _p(ws), nb,
              _stream())
    return loss, dl, nll, cnt


# ------------------------------------------------------------------------------------------------
# latent prior (GatedPixelCNN): incremental sampling, the per-row column walk
# ------------------------------------------------------------------------------------------------
def prior_walk_weight_floats(dim, n_layers, input_dim) -> int:
    """Floats of the walk's packed weight blob (layout: include/nsg.h, nsg_prior_walk); 0 outside the kernel's envelope."""
    return int(_lib.query("nsg_prior_walk_weight_floats", dim, n_layers, input_dim))


def _prior_walk_extents(fn, w, emb, cond, vh, e_row, H, row, tensors):
    """The checks prior_walk and prior_walk_ctl share; tensors: (tensor or None, name, dtype, trailing shape after (B, H, W)).
    Returns (B, W, dim, L, K)."""
    for t, nm in ((w, "w"), (emb, "emb"), (cond, "cond"), (vh, "vh")):
        _chk(t, nm)
    K, dim = emb.shape
    L, B = cond.shape[0], cond.shape[1]
    W = e_row.shape[1]
    if tuple(cond.shape) != (L, B, 2 * dim) or tuple(vh.shape) != (L, B, 1, W, 2 * dim):
        raise _lib.NsgError(f"{fn}: cond {tuple(cond.shape)} / vh {tuple(vh.shape)} do not match emb {tuple(emb.shape)}")
    if w.numel() != prior_walk_weight_floats(dim, L, K):
        raise _lib.NsgError(f"{fn}: weight blob of {w.numel()} floats, expected {prior_walk_weight_floats(dim, L, K)}")
    if not e_row.is_cuda or e_row.dtype != torch.float32 or tuple(e_row.shape) != (B, W, dim) or e_row.stride()[1:] != (dim, 1):
        raise _lib.NsgError(f"{fn}: e_row must be fp32 (B, W, dim) = {(B, W, dim)} with rows of dim contiguous floats")
    for t, nm, dt, tail, *lead in tensors:          # lead: the leading extent where it is not B (prior_walk_cfg's pairs)
        if t is not None:
            _chk(t, nm, dt)
            if tuple(t.shape) != (lead[0] if lead else B, H, W) + tail:
                raise _lib.NsgError(f"{fn}: {nm} {tuple(t.shape)}, expected {(lead[0] if lead else B, H, W) + tail}")
    if not 0 <= row < H:
        raise _lib.NsgError(f"{fn}: row {row} outside 0 .. {H - 1}")
    return B, W, dim, L, K


def prior_walk(w, emb, cond, vh, e_row, H, row, u=None, x_in=None, codes=None, logits=None):
    """Walk row `row` of a (B, H, W) code grid (nsg_prior_walk).  w: packed blob; emb (K, dim); cond (L, B, 2 dim); vh
    (L, B, 1, W, 2 dim); e_row (B, W, dim), any clip stride, receives the embedding of the row's codes; exactly one of u
    (B, H, W) fp32 (sampling: codes (B, H, W) int64 is written) and x_in (B, H, W) int64 (teacher-forced); logits
    (B, H, W, K) optional."""
    if (u is None) == (x_in is None):
        raise _lib.NsgError("prior_walk: exactly one of u (sampling) and x_in (teacher-forced)")
    if u is not None and codes is None:
        raise _lib.NsgError("prior_walk: sampling needs a codes output")
    K = emb.shape[0]
    B, W, dim, L, K = _prior_walk_extents("prior_walk", w, emb, cond, vh, e_row, H, row, (
        (u, "u", torch.float32, ()), (x_in, "x_in", torch.int64, ()), (codes, "codes", torch.int64, ()), (logits, "logits", torch.float32, (K,))))
    _lib.call("nsg_prior_walk", _p(w), _p(emb), _p(cond), _p(vh), _p(u), _p(x_in), _p(codes), _p(e_row), e_row.stride(0), _p(logits), B, H, W, dim, L,
              K, row, _stream())


def prior_walk_ctl(w, emb, cond, vh, e_row, H, row, u, codes, x_in=None, keep=None, logits=None, temperature=1.0, top_k=0, top_p=1.0):
    """prior_walk's sampling mode with a controlled pick (nsg_prior_walk_ctl; the rule is in include/nsg.h): temperature > 0,
    top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off), and kept codes: where keep (B, H, W) bool or uint8 is non-zero the code
    is x_in's (B, H, W) int64 and u is not consulted.  x_in and keep come together.  u (B, H, W) fp32 and codes (B, H, W)
    int64 are required; logits (B, H, W, K) optional."""
    if u is None or codes is None:
        raise _lib.NsgError("prior_walk_ctl: u and codes are required")
    if (x_in is None) != (keep is None):
        raise _lib.NsgError("prior_walk_ctl: x_in and keep come together")
    if keep is not None and keep.dtype not in (torch.bool, torch.uint8):
        raise _lib.NsgError(f"prior_walk_ctl: keep must be bool or uint8, got {keep.dtype}")
    temperature, top_p = float(temperature), float(top_p)
    if not (math.isfinite(temperature) and temperature > 0 and 0 < top_p <= 1) or int(top_k) != top_k or top_k < 0:
        raise _lib.NsgError(f"prior_walk_ctl: temperature {temperature} (finite, > 0), top_k {top_k} (integer >= 0) or top_p {top_p} "
                            "(in (0, 1]) out of range")
    K = emb.shape[0]
    B, W, dim, L, K = _prior_walk_extents("prior_walk_ctl", w, emb, cond, vh, e_row, H, row, (
        (u, "u", torch.float32, ()), (x_in, "x_in", torch.int64, ()), (keep, "keep", None, ()), (codes, "codes", torch.int64, ()),
        (logits, "logits", torch.float32, (K,))))
    _lib.call("nsg_prior_walk_ctl", _p(w), _p(emb), _p(cond), _p(vh), _p(u), _p(x_in), _p(keep), _p(codes), _p(e_row), e_row.stride(0), _p(logits), B,
              H, W, dim, L, K, row, temperature, min(int(top_k), 2 ** 31 - 1), top_p, _stream())


def prior_walk_cfg(w, emb, cond, vh, e_row, H, row, u, codes, guidance, x_in=None, keep=None, logits=None, temperature=1.0, top_k=0,
                   top_p=1.0):
    """prior_walk_ctl under classifier-free guidance (nsg_prior_walk_cfg; the rule is in include/nsg.h).  cond, vh and e_row
    hold B = 2P clips: clips 2p and 2p + 1 are pair p, the conditional branch (the real label's rows) and the unconditional
    one (the null label's).  u (P, H, W) fp32, codes (P, H, W) int64 and the optional x_in / keep (P, H, W) are per pair;
    logits (B, H, W, K) optional receives each branch's raw logits.  The pick runs on l_c + guidance * (l_c - l_u), guidance
    in [0, 1024], and both clips of a pair continue from the pair's code."""
    if u is None or codes is None:
        raise _lib.NsgError("prior_walk_cfg: u and codes are required")
    if (x_in is None) != (keep is None):
        raise _lib.NsgError("prior_walk_cfg: x_in and keep come together")
    if keep is not None and keep.dtype not in (torch.bool, torch.uint8):
        raise _lib.NsgError(f"prior_walk_cfg: keep must be bool or uint8, got {keep.dtype}")
    temperature, top_p, guidance = float(temperature), float(top_p), float(guidance)
    if not (math.isfinite(temperature) and temperature > 0 and 0 < top_p <= 1) or int(top_k) != top_k or top_k < 0:
        raise _lib.NsgError(f"prior_walk_cfg: temperature {temperature} (finite, > 0), top_k {top_k} (integer >= 0) or top_p {top_p} "
                            "(in (0, 1]) out of range")
    if not 0 <= guidance <= 1024:                   # NaN fails both comparisons
        raise _lib.NsgError(f"prior_walk_cfg: guidance {guidance} outside [0, 1024]")
    if cond.dim() != 3 or cond.shape[1] % 2 != 0:
        raise _lib.NsgError(f"prior_walk_cfg: cond {tuple(cond.shape)} must hold an even number of clips (pairs of branches)")
    K, P = emb.shape[0], cond.shape[1] // 2
    B, W, dim, L, K = _prior_walk_extents("prior_walk_cfg", w, emb, cond, vh, e_row, H, row, (
        (u, "u", torch.float32, (), P), (x_in, "x_in", torch.int64, (), P), (keep, "keep", None, (), P),
        (codes, "codes", torch.int64, (), P), (logits, "logits", torch.float32, (K,))))
    _lib.call("nsg_prior_walk_cfg", _p(w), _p(emb), _p(cond), _p(vh), _p(u), _p(x_in), _p(keep), _p(codes), _p(e_row), e_row.stride(0), _p(logits), B,
              H, W, dim, L, K, row, temperature, min(int(top_k), 2 ** 31 - 1), top_p, guidance, _stream())


def prepared_conv_forward(d: ConvDesc, x, w_fwd, bias, y, flags=0):
    """nsg_conv_forward on fixed tensors, checked once: returns a no-argument callable that launches it on the current
    stream (a loop that runs the same layer once per row skips conv_forward's per-call checks and allocations)."""
    _chk(x, "x", _in_dtype(d)); _chk(y, "y", _out_dtype(d, flags))
    if tuple(x.shape) != (d.B, d.IH, d.IW, d.C_in) or tuple(y.shape) != (d.B, d.OH, d.OW, d.C_out):
        raise _lib.NsgError(f"prepared_conv_forward: x {tuple(x.shape)} / y {tuple(y.shape)} do not match descriptor {d.key()}")
    ws, nb = _ws(x.device, "nsg_conv_workspace_bytes", byref(d))
    keep = (d, x, w_fwd, bias, y, ws)          # the closure owns every buffer whose address it passes
    args = (byref(d), _p(x), _p(w_fwd), _p(bias), _p(y), flags, _p(ws), nb)
    return lambda: (keep, _lib.call("nsg_conv_forward", *args, _stream()))


def prepared_gated_activation(x, cond, y):
    """nsg_gated_activation_forward on fixed tensors (x (..., 2C), cond (B, 2C), y (..., C)), checked once: a callable."""
    _chk(x, "x"); _chk(cond, "cond"); _chk(y, "y")
    C2 = x.shape[-1]
    M = x.numel() // C2
    if cond.shape[-1] != C2 or M % cond.shape[0] != 0 or y.numel() != M * (C2 // 2):
        raise _lib.NsgError(f"prepared_gated_activation: x {tuple(x.shape)}, cond {tuple(cond.shape)}, y {tuple(y.shape)}")
    keep = (x, cond, y)
    args = (_p(x), _p(cond), _p(y), M, C2 // 2, M // cond.shape[0])
    return lambda: (keep, _lib.call("nsg_gated_activation_forward", *args, _stream()))
