"""Host restatements of the F0-conditioned decoder's definitions (include/nsg.h: nsg_f0_bins, nsg_add_cond, nsg_column_sum).

  * bins_f64: the definition of the bins in fp64 (numpy) -- what the kernel is judged against;
  * bins_f32: the same in fp32 in the kernel's stated operation order -- what the kernel computes, up to the last-place
    differences of two log2 implementations;
  * decided: the columns on which the two must agree: those whose fp64 u lies at least `margin` bin widths from every integer
    (fp32 places u within about 1e-5 bin widths at 32 bins over 65 .. 500 Hz: a few ulps of a log2 F0 near 8, times n_bins / span);
  * affine_f64: audio.f0_affine's rows from a contour, in fp64;
  * conditioned_oracle: the CPU autograd definition of the conditioned training step, on the oracle's encoder / quantiser /
    decoder, as tests/test_gpu_model.py's _speaker_oracle is for the speaker table alone."""
import numpy as np


def _columns(f0, frames, W):
    f0 = np.asarray(f0, dtype=np.float32)
    B, T = f0.shape
    assert T >= 4 * W
    fr = np.full(B, T, dtype=np.int64) if frames is None else np.clip(np.asarray(frames, dtype=np.int64), 0, T)
    cols = f0[:, :4 * W].reshape(B, W, 4)
    t = np.arange(4 * W).reshape(1, W, 4)
    valid = (cols > 0) & (t < fr[:, None, None])
    return cols, valid


def bins_f64(f0, W, n_bins, fmin, fmax, frames=None, affine=None):
    """-> (bins (B, W) int64, logf (B, W) fp64, u (B, W) fp64 (NaN where unvoiced), voiced (B, W) bool)."""
    cols, valid = _columns(f0, frames, W)
    n = valid.sum(-1)
    l = np.where(valid, np.log2(np.where(valid, cols, 1.0).astype(np.float64)), 0.0)
    voiced = n >= 2
    mean = l.sum(-1) / np.maximum(n, 1)
    if affine is not None:
        a = np.asarray(affine, dtype=np.float64)
        mean = a[:, 2:3] + (mean - a[:, 0:1]) * a[:, 1:2]
    lo, hi = np.log2(np.float64(np.float32(fmin))), np.log2(np.float64(np.float32(fmax)))
    u = (mean - lo) * n_bins / (hi - lo)
    bins = np.where(voiced, 1 + np.clip(np.floor(u), 0, n_bins - 1), 0).astype(np.int64)
    return bins, np.where(voiced, mean, 0.0), np.where(voiced, u, np.nan), voiced


def bins_f32(f0, W, n_bins, fmin, fmax, frames=None, affine=None):
    """The kernel's arithmetic: fl32(log2((double)f0)) summed in frame order in fp32, / (float)n, the affine move as difference,
    product, sum, then u = ((l' - lo) * (float)n_bins) / span with lo = fl32(log2 fmin), span = fl32(log2 fmax) - lo.
    -> (bins (B, W) int64, logf (B, W) fp32)."""
    f32 = np.float32
    cols, valid = _columns(f0, frames, W)
    n = valid.sum(-1)
    l = np.log2(np.where(valid, cols, 1.0).astype(np.float64)).astype(f32)
    s = np.zeros(n.shape, dtype=f32)
    for t in range(4):
        s = np.where(valid[..., t], (s + l[..., t]).astype(f32), s)
    voiced = n >= 2
    mean = (s / np.maximum(n, 1).astype(f32)).astype(f32)
    if affine is not None:
        a = np.asarray(affine, dtype=f32)
        mean = (a[:, 2:3] + ((mean - a[:, 0:1]).astype(f32) * a[:, 1:2]).astype(f32)).astype(f32)
    lo = f32(np.log2(np.float64(f32(fmin))))
    span = f32(f32(np.log2(np.float64(f32(fmax)))) - lo)
    u = (((mean - lo).astype(f32) * f32(n_bins)).astype(f32) / span).astype(f32)
    b = np.minimum(np.maximum(np.floor(u), f32(0)), f32(n_bins) - f32(1))
    return np.where(voiced, 1 + b, 0).astype(np.int64), np.where(voiced, mean, f32(0)).astype(f32)


def decided(u64, margin=1e-4):
    """Columns whose bin no fp32 evaluation may move: u at least `margin` bin widths from every integer (False where u is NaN)."""
    u = np.asarray(u64, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(u - np.round(u)) >= margin


def logf0_sums_f64(f0, frames=None):
    """audio.logf0_sums in numpy: (B, 3) fp64 (n_voiced, sum log2 f0, sum (log2 f0)^2) over the voiced frames below frames[b]."""
    f0 = np.asarray(f0, dtype=np.float32)
    B, T = f0.shape
    fr = np.full(B, T, dtype=np.int64) if frames is None else np.asarray(frames, dtype=np.int64)
    valid = (f0 > 0) & (np.arange(T)[None, :] < fr[:, None])
    l = np.where(valid, np.log2(np.where(valid, f0, 1.0).astype(np.float64)), 0.0)
    return np.stack((valid.sum(1).astype(np.float64), l.sum(1), (l * l).sum(1)), axis=1)


def affine_f64(sums, target_mean, target_std, min_var=1e-12):
    """audio.f0_affine in numpy fp64 -> (B, 3) fp32 rows (mu_src, ratio, mu_tgt)."""
    sums = np.asarray(sums, dtype=np.float64)
    n, s1, s2 = sums[:, 0], sums[:, 1], sums[:, 2]
    mt = np.broadcast_to(np.asarray(target_mean, dtype=np.float64), n.shape)
    st = np.broadcast_to(np.asarray(target_std, dtype=np.float64), n.shape)
    n1 = np.maximum(n, 1)
    mu = np.where(n > 0, s1 / n1, mt)
    var = np.where(n > 0, s2 / n1 - (s1 / n1) ** 2, 0.0)
    spread = (n >= 2) & (var > min_var)
    ratio = np.where(spread, st / np.sqrt(np.where(spread, var, 1.0)), 1.0)
    return np.stack((mu, ratio, mt), axis=1).astype(np.float32)


def conditioned_oracle(st0, c, g, bins):
    """CPU definition of the speaker- and F0-conditioned step: oracle encoder / quantiser / decoder with the clip's speaker row
    added to every latent pixel and the column's F0 row to every pixel of that column; autograd gives both tables' gradients.
    st0: the model's state_dict (CPU); c (B, 1, 80, T); g (B,) int64 or None; bins (B, W) int64.
    -> (loss_recons, loss_vq, idx, grad speaker table or None, grad F0 table)."""
    import torch
    from oracle import vqvae_oracle as O
    ost = O.clone_state({k: v for k, v in st0.items() if not k.startswith(("speaker_embedding", "f0_embedding"))})
    f0emb = st0["f0_embedding.weight"].clone().requires_grad_(True)
    spk = st0["speaker_embedding.weight"].clone().requires_grad_(True) if g is not None else None
    z_e = O.encoder(c, ost, True, {})
    zq_st, zq_bar, idx = O.straight_through(z_e, ost["codebook.embedding.weight"])
    zdec = zq_st
    if spk is not None:
        zdec = zdec + spk[g][:, :, None, None]
    zdec = zdec + f0emb[bins].permute(0, 2, 1)[:, :, None, :]
    x_t = O.decoder(zdec, ost, True, {})
    lr_, lv, lc = O.loss_terms(c, x_t, z_e, zq_bar)
    grads = torch.autograd.grad(lr_ + lv + lc, [f0emb] + ([spk] if spk is not None else []))
    return lr_, lv, idx, (grads[1] if spk is not None else None), grads[0]
