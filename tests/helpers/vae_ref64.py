"""The fp64 yardstick of the VAE's library pieces: the Gaussian latent (csrc/vae_latent.hip) and the stride-1 transposed
convolution (csrc/conv_api.hip, K_CONVT_S1).  Plain torch on the CPU.  Every function widens what it is given to float64, so a
caller passes the operands as the kernel sees them: fp32 values (the statistics ops.bn_stats returned included)."""
import torch
import torch.nn.functional as F


U32 = 2.0 ** -24                    # unit roundoff of fp32


def f64(t):
    return None if t is None else t.detach().to("cpu").double()


# ----------------------------------------------------------------------------------------------------------------------
# the latent: rows [M][2Z], channels [0, Z) mu, [Z, 2Z) logvar, both AFTER the BatchNorm's affine map of h
# ----------------------------------------------------------------------------------------------------------------------
def latent_parts(h, mean, invstd, gamma, beta):
    """-> mu, lv, sigma, xhat ([M][Z], [M][Z], [M][Z], [M][2Z])."""
    h, mean, invstd = f64(h), f64(mean), f64(invstd)
    y = (h - mean) * (invstd * f64(gamma)) + f64(beta)
    Z = y.shape[1] // 2
    mu, lv = y[:, :Z], y[:, Z:]
    return mu, lv, torch.exp(0.5 * lv), (h - mean) * invstd


def latent_forward(h, mean, invstd, gamma, beta, eps):
    """-> z [M][Z], kl (a 0-d tensor), sum |term| of the kl mean (the scale its fp32 bound refers to)."""
    mu, lv, sigma, _ = latent_parts(h, mean, invstd, gamma, beta)
    terms = 0.5 * (mu * mu + sigma * sigma - 1.0 - lv)
    M = mu.shape[0]
    return mu + sigma * f64(eps), terms.sum() / M, terms.abs().sum() / M


def latent_backward(h, mean, invstd, gamma, beta, eps, dz, kl_scale=1.0, kl_grad=1.0):
    """-> dy [M][2Z], dgamma, dbeta [2Z]; sum |term| per column of the two sums; mag [M][2Z], the magnitude of the terms each dy
    element is formed from (|dz| + |s mu|;  |dz sigma eps| / 2 + |s| (sigma^2 + 1) / 2); own [M][2Z], the rounding an fp32 dy
    element carries before it is summed: U32 * mag * (8 + 3 L), eight roundings of the expression itself (as the BatchNorm
    envelope counts them for dx_colsum) and, in the logvar half, the three roundings of lv, each up to U32 * L with L =
    |h - mean| |invstd gamma| + |beta| the magnitude lv is formed from, which move sigma^2 by that much RELATIVE (L = 0 for mu)."""
    mu, lv, sigma, xhat = latent_parts(h, mean, invstd, gamma, beta)
    eps, dz = f64(eps), f64(dz)
    Z = mu.shape[1]
    s = kl_scale * kl_grad / mu.shape[0]
    dy = torch.cat([dz + s * mu, 0.5 * dz * sigma * eps + 0.5 * s * (sigma * sigma - 1.0)], dim=1)
    mag = torch.cat([dz.abs() + abs(s) * mu.abs(), 0.5 * (dz * sigma * eps).abs() + 0.5 * abs(s) * (sigma * sigma + 1.0)], dim=1)
    L = (f64(h) - f64(mean)).abs() * (f64(invstd) * f64(gamma)).abs() + f64(beta).abs()
    L[:, :Z] = 0.0
    own = U32 * mag * (8.0 + 3.0 * L)
    return dy, (dy * xhat).sum(0), dy.sum(0), (dy * xhat).abs().sum(0), dy.abs().sum(0), mag, own, xhat


def latent_autograd(h, mean, invstd, gamma, beta, eps, dz, kl_scale=1.0, kl_grad=1.0):
    """The same gradient from torch.autograd over the reference's own expressions (models.py:103-112), the BatchNorm's output
    taken as the leaf: what test_vae_host.py holds latent_backward to."""
    h, mean, invstd = f64(h), f64(mean), f64(invstd)
    y = ((h - mean) * (invstd * f64(gamma)) + f64(beta)).requires_grad_(True)
    mu, lv = y.chunk(2, dim=1)
    q = torch.distributions.Normal(mu, (0.5 * lv).exp())
    p = torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(lv))
    kl = torch.distributions.kl_divergence(q, p).sum(1).mean()
    z = mu + (0.5 * lv).exp() * f64(eps)
    (z * f64(dz)).sum().add(kl_scale * kl_grad * kl).backward()
    return z.detach(), kl.detach(), y.grad


# ----------------------------------------------------------------------------------------------------------------------
# ConvTranspose2d(C_in, C_out, k, 1, pad); tensors NCHW here (the tests permute), weight (C_in, C_out, k, k)
# ----------------------------------------------------------------------------------------------------------------------
def convt_forward(x, w, bias, pad):
    return F.conv_transpose2d(f64(x), f64(w), f64(bias), stride=1, padding=pad)


def convt_backward(x, w, dy, pad):
    """-> dx, dw, dbias by autograd, and sum |term| of every dw / dbias element (the scale their fp32 bounds refer to):
    the same contraction over |x| and |dy|."""
    x, w, dy = f64(x).requires_grad_(True), f64(w).requires_grad_(True), f64(dy)
    b = torch.zeros(w.shape[1], dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(x, w, b, stride=1, padding=pad).mul(dy).sum().backward()
    xa, wa = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    F.conv_transpose2d(xa, wa, None, stride=1, padding=pad).mul(dy.abs()).sum().backward()
    return x.grad, w.grad, b.grad, wa.grad, dy.abs().sum((0, 2, 3))
