"""ConvTranspose2d(C_in, C_out, k, 1, pad) through nsg_conv_* (csrc/conv_api.hip, K_CONVT_S1) against the fp64 yardstick
tests/helpers/vae_ref64.py: forward with bias, forward_bnstats, the data gradient and the weight / bias gradients, for the VAE
decoder's two geometries (k = 3 and 5, pad = 0) and two padded ones, channel counts below, at and off a multiple of the GEMM's
32-wide K chunk, and inputs down to ONE column (the VAE's smallest latent grid).

The layer has no kernel of its own: the forward is the stride-1 gather with pad' = k - 1 - pad over taps the packer flipped and
swapped, the data gradient the plain gather, the weight gradient the Conv2d kernel with x and dy in each other's roles.  A wrong
flip, swap or pad' is an O(1) error on every element, far outside the bounds.

Bounds (the classes of tests/test_gpu_bn_envelope.py; none is tuned against the kernels):
  element-wise outputs   1e-5 of the output's largest magnitude (fp32 MFMA, at most 7 * 7 * 20 = 980 products per element)
  dw, dbias              2e-5 * sum |term| of the element
  mean / invstd          mean: 1e-5 |mean| + 2e-6 std + 1e-6; invstd: rtol 2e-5

Largest error / bound per class as measured on an MI355X (also DESIGN.md, "The continuous VAE"): element-wise 0.088 (k=5 pad=0
12->20 14x5 dgrad), dw / dbias 0.012, mean 0.048, invstd 0.021, running statistics 0.033."""
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from tests.helpers import vae_ref64 as R  # noqa: E402

DEV = "cuda:0"
B = 2
GEOMS = [(3, 0), (5, 0), (3, 1), (7, 3)]
CHANNELS = [(4, 8), (8, 4), (12, 20)]
INPUTS = [(14, 1), (14, 5), (16, 3)]
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


def _poison(like):
    t = torch.full(like.shape, float("nan"), dtype=like.dtype, device=like.device)
    del t


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.fixture(scope="module", params=list(itertools.product(GEOMS, CHANNELS, INPUTS)),
                ids=lambda p: f"k{p[0][0]}p{p[0][1]}-{p[1][0]}to{p[1][1]}-{p[2][0]}x{p[2][1]}")
def case(request):
    (k, pad), (ci, co), (ih, iw) = request.param
    g = torch.Generator().manual_seed(1000 * k + 100 * pad + 10 * ci + ih + iw)
    c = types.SimpleNamespace(k=k, pad=pad, ci=ci, co=co, tag=f"k={k} pad={pad} {ci}->{co} {ih}x{iw}")
    c.x = torch.randn(B, ci, ih, iw, generator=g)
    c.w = torch.randn(ci, co, k, k, generator=g) * 0.2
    c.bias = torch.randn(co, generator=g)
    c.d = ops.conv_desc(B, ih, iw, ci, co, k, 1, pad, transposed=True)
    assert (c.d.OH, c.d.OW) == (ih + k - 1 - 2 * pad, iw + k - 1 - 2 * pad)
    c.dy = torch.randn(B, co, c.d.OH, c.d.OW, generator=g)
    c.xg, c.dyg, c.wg, c.biasg = nhwc(c.x), nhwc(c.dy), c.w.to(DEV), c.bias.to(DEV)
    c.wf, c.wd = ops.pack_weights(c.d, c.wg)
    c.y64 = R.convt_forward(c.x, c.w, c.bias, pad)
    return c


def test_forward_with_bias(case):
    c = case
    _poison(c.dyg)
    y = ops.conv_forward(c.d, c.xg, c.wf, c.biasg)
    _within("element-wise", nchw(y), c.y64, 1e-5 * float(c.y64.abs().max()), c.tag + " forward")
    assert torch.equal(ops.conv_forward(c.d, c.xg, c.wf, c.biasg), y)


def test_forward_bnstats(case):
    c = case
    rm, rv = torch.zeros(c.co, device=DEV), torch.ones(c.co, device=DEV)
    _poison(c.dyg)
    y, mean, invstd = ops.conv_forward_bnstats(c.d, c.xg, c.wf, c.biasg, running_mean=rm, running_var=rv)
    assert torch.equal(y, ops.conv_forward(c.d, c.xg, c.wf, c.biasg))
    rows = c.y64.permute(0, 2, 3, 1).reshape(-1, c.co)
    M = rows.shape[0]
    mean64 = rows.mean(0)
    m2 = ((rows - mean64) ** 2).sum(0)
    invstd64 = 1.0 / torch.sqrt(m2 / M + 1e-5)
    _within("mean", mean, mean64, 1e-5 * mean64.abs() + 2e-6 / invstd64 + 1e-6, c.tag + " mean")
    _within("invstd", invstd, invstd64, 2e-5 * invstd64, c.tag + " invstd")
    rm64, rv64 = 0.1 * mean64, 0.9 + 0.1 * m2 / (M - 1)
    _within("running statistics", rm, rm64, 1e-5 * rm64.abs() + 1e-6, c.tag + " running_mean")
    _within("running statistics", rv, rv64, 1e-5 * rv64.abs() + 1e-6, c.tag + " running_var")


def test_dgrad(case):
    c = case
    dx64, _, _, _, _ = R.convt_backward(c.x, c.w, c.dy, c.pad)
    _poison(c.xg)
    dx = ops.conv_dgrad(c.d, c.dyg, c.wd)
    _within("element-wise", nchw(dx), dx64, 1e-5 * float(dx64.abs().max()), c.tag + " dgrad")


def test_wgrad_with_dbias(case):
    c = case
    _, dw64, db64, t_dw, t_db = R.convt_backward(c.x, c.w, c.dy, c.pad)
    nan = float("nan")
    dw, db = ops.conv_wgrad(c.d, c.xg, c.dyg, c.w.shape, dw=torch.full(c.w.shape, nan, device=DEV), dbias=torch.full((c.co,), nan, device=DEV))
    _within("fp32 sums", dw, dw64, 2e-5 * t_dw, c.tag + " dw")
    _within("fp32 sums", db, db64, 2e-5 * t_db, c.tag + " dbias")
    dw2, db2 = ops.conv_wgrad(c.d, c.xg, c.dyg, c.w.shape)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


def test_report_worst_ratios():
    """Not a check: prints the largest error / bound each class reached in this run (pytest -s shows it)."""
    for cls, (ratio, where) in sorted(WORST.items()):
        print(f"convt stride-1  {cls:20s} {ratio:.3f}  at {where}")
