"""The Gaussian-latent kernels (csrc/vae_latent.hip) over their envelope against the fp64 yardstick tests/helpers/vae_ref64.py.

Z: 4 (one channel group per half: 255 of 256 threads are row groups), 32, 36 (2Z / 4 = 18 does not divide 256: idle threads),
128.  M: 1 and 28 (the VAE's smallest latent grid at 2 clips), and a value on each side of every boundary of the reduction
geometry -- both kernels run one block per slab of nsg_bn_slab_geom(M) (slabs of >= 64 rows, at most 1024 of them):
    64 | 65            one block | two
    4096 | 4097        64 slabs = one lap of the KL sum's one-wave closer | a second lap
    16384 | 16385      256 slabs = one record per thread in bn.hip's finaliser | two
    65536 | 65537      1024 slabs of 64 rows | the slab cap: 65 rows per slab, 1009 slabs
    70001              69 rows per slab, the last slab short
There is no grid stride: a block owns one slab and its threads stride the slab's rows by 256 / (channels / 4) row groups, which
is more than a slab's 64 rows at Z = 4 (idle row groups) and fewer at Z = 128.

Inputs: h ~ N(0, 1), mean / invstd from ops.bn_stats (the fp32 values the kernels are handed; the reference widens those), gamma
~ U(0.5, 1.5), beta ~ U(-0.3, 0.3), eps, dz ~ N(0, 1); beta of logvar channel 1 is -20 and of logvar channel 2 is +20 (sigma^2
up to e^24: no clamping anywhere).

Bounds against fp64 (the classes of tests/test_gpu_bn_envelope.py; none is tuned against the kernels), scales per CHANNEL so
the +-20 channels cannot hide the others:
  z, dy               1e-5 of the channel's scale.  The scale is the largest magnitude of the terms an element is formed from
                      over the channel's rows -- |mu| + |sigma eps| for z, |dz| + |s mu| for dy_mu, |dz sigma eps| / 2 +
                      |s| (sigma^2 + 1) / 2 for dy_lv -- not of the result: at M = 1 a channel is ONE element, and mu + sigma eps
                      cancels to 1 % of its terms in one channel of a hundred, where 1e-5 of the result would ask for 1e-7 of
                      the terms, the unit roundoff itself.
  kl                  2e-5 * sum |term| (a double accumulation of terms formed in fp32)
  dgamma, dbeta       2e-5 * sum |term| for the fp32 chains (below 300 adds), plus the roundings of the kernel's own fp32 dy
                      that it sums: vae_ref64.latent_backward's `own`, U32 * (8 + 3 L) of the magnitudes each dy element is
                      formed from, as the BatchNorm envelope grants dx_colsum 8 * 2^-24 of them.  Without that part the bound
                      is relative to |dy| where dy cancels, which no fp32 kernel meets: at M = 1 a column sum is ONE dy, and
                      the first run on an MI355X missed 2e-5 |dy| by 4.4x in one column at M = 1, Z = 128 while dy met its own bound.

Largest error / bound per class as measured on an MI355X (also DESIGN.md, "The continuous VAE"): z 0.072 and dy 0.125 (both at
M=70001 Z=4), kl 0.013 (M=28 Z=36), dgamma / dbeta 0.102 (M=1 Z=128 dbeta)."""
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from tests.helpers import vae_ref64 as R  # noqa: E402

DEV = "cuda:0"
ZS = [4, 32, 36, 128]
MS = [1, 28, 64, 65, 4096, 4097, 16384, 16385, 65536, 65537, 70001]
NAN = float("nan")
WORST = {}


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _within(cls, got, want, bound, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got.detach().double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    _note(cls, ratio, what)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def _nan(*shape):
    """An output allocated over poison: an element the kernel does not write stays NaN."""
    return torch.full(shape, NAN, device=DEV)


@pytest.fixture(scope="module", params=list(itertools.product(MS, ZS)), ids=lambda p: f"M{p[0]}-Z{p[1]}")
def case(request):
    M, Z = request.param
    g = torch.Generator().manual_seed(7 * M + Z)
    c = types.SimpleNamespace(M=M, Z=Z, tag=f"M={M} Z={Z}")
    c.h = torch.randn(M, 2 * Z, generator=g)
    c.gamma = torch.rand(2 * Z, generator=g) + 0.5
    c.beta = torch.rand(2 * Z, generator=g) * 0.6 - 0.3
    c.beta[Z + 1], c.beta[Z + 2] = -20.0, 20.0
    c.eps = torch.randn(M, Z, generator=g)
    c.dz = torch.randn(M, Z, generator=g)
    for n in ("h", "gamma", "beta", "eps", "dz"):
        setattr(c, n + "g", getattr(c, n).to(DEV))
    c.mean, c.invstd = ops.bn_stats(c.hg, 2 * Z)
    c.args = (c.hg, c.mean, c.invstd, c.gammag, c.betag, c.epsg)
    c.ref = (c.h, c.mean, c.invstd, c.gamma, c.beta, c.eps)
    return c


def _forward(c):
    return ops.vae_latent_forward(*c.args, z=_nan(c.M, c.Z), kl=_nan(1))


def _backward(c, kl_scale=1.0, kl_grad=None):
    return ops.vae_latent_backward(*c.args, c.dzg, kl_scale=kl_scale, kl_grad=kl_grad, dy=_nan(c.M, 2 * c.Z), dgamma=_nan(2 * c.Z),
                                   dbeta=_nan(2 * c.Z))


def test_forward(case):
    c = case
    z, kl = _forward(c)
    z2, kl2 = _forward(c)
    assert torch.equal(z, z2) and torch.equal(kl, kl2), "two runs of the same call differ"
    mu, lv, sigma, _ = R.latent_parts(*c.ref[:5])
    z64, kl64, kl_terms = R.latent_forward(*c.ref)
    scale = (mu.abs() + (sigma * c.eps.double()).abs()).amax(0)
    _within("z", z, z64, 1e-5 * scale, c.tag + " z")
    _within("kl", kl[0], kl64, 2e-5 * kl_terms, c.tag + " kl")


@pytest.mark.parametrize("kl_scale,kl_grad", [(1.0, None), (0.25, None), (1.0, -1.7), (0.0, None)], ids=["plain", "scale", "grad", "no-kl"])
def test_backward(case, kl_scale, kl_grad):
    c = case
    kg = None if kl_grad is None else torch.tensor([kl_grad], device=DEV)
    dy, dg, db = _backward(c, kl_scale, kg)
    for a, b in zip(_backward(c, kl_scale, kg), (dy, dg, db)):
        assert torch.equal(a, b), "two runs of the same call differ"
    # the sums are nsg_bn_backward_sums's over the stored dy, bit for bit, so nsg_bn_backward_apply finishes the BatchNorm
    dg2, db2 = ops.bn_backward_sums(c.hg, dy, c.mean, c.invstd, c.gammag)
    assert torch.equal(dg, dg2) and torch.equal(db, db2)
    dy64, dg64, db64, t_dg, t_db, mag, own, xhat = R.latent_backward(*c.ref, c.dz, kl_scale, 1.0 if kl_grad is None else kl_grad)
    _within("dy", dy, dy64, 1e-5 * mag.amax(0), c.tag + " dy")
    _within("fp32 sums", db, db64, 2e-5 * t_db + own.sum(0), c.tag + " dbeta")
    _within("fp32 sums", dg, dg64, 2e-5 * t_dg + (own * xhat.abs()).sum(0), c.tag + " dgamma")


def test_null_kl_grad_is_one(case):
    c = case
    one = torch.ones(1, device=DEV)
    for a, b in zip(_backward(c, 0.7, None), _backward(c, 0.7, one)):
        assert torch.equal(a, b)


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[vae latent] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
