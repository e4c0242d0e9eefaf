"""The fused output layer BatchNorm -> ReLU -> ConvTranspose2d(C, 1, 4, 2, 1) [-> Tanh] [-> reconstruction loss] (second half of
csrc/c1_mfma.hip: bnrelu_dots_kernel and the SWAP = true forms of c1m_bwd_sums_kernel / c1m_bwd_wgrad_kernel; the col2im and loss
epilogue of csrc/conv_api.hip) over its envelope, against the fp64 yardstick tests/helpers/fused_ref64.py.

C: 32, 64, 96, 128, 256 -- all of nsg_bn_relu_c1convt_supported.  u is [B][H][W][C] bf16, the image [B][2H][2W] fp32.  The forward's
dots kernel works on flat 128-row blocks of M = B H W, at most 1024 of them (512 at C = 256); the backward passes on 64-pixel tiles
of one row, B H ceil(W / 64) tiles over at most 1024 blocks.  Shapes (B, H, W):
    (1,1,1)  (2,3,1)                   one pixel with halo on every side; one column
    (1,1,63 | 64 | 65)                 the 64-pixel tile edge in one row
    (2,5,130)                          a ragged third tile
    (1,2,64)  (1,3,43)                 M = 128 exactly; M = 129
    (1,1024,3) | (1,1025,3) (5,205,1)  1024 backward tiles: at the block cap | 1025: just past it
    (1,2048,64) | (1,131073,1)         the forward's block cap, M = 131072 | 131073 (C = 256: (1,1024,64) | (1,65537,1))
every shape at C = 128, the tile-edge and cap shapes at C = 256 and C = 32, three shapes at C = 64 and C = 96
(fused_ref64.CASES_OUT; tests/test_fused_ref_host.py derives the table from the constants and checks the inputs on the CPU).  The
loss form runs T = 2W, 2W + 1, 2W + 37 at (2,3,1), (1,1,65), (2,5,130), once with the image requested and once with dbias.

Inputs as tests/test_gpu_ops.py's: u ~ N(0.5, 1.5^2) as bf16, w ~ N(0, 0.2^2), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.3^2), dy ~ N(0, 1);
channel 1 has beta = -8 (the ReLU passes almost nothing), channel 2 is 6 +- 0.2 (mean >> std).

Bounds against fp64 (derived in fused_ref64.py, none tuned against the kernels):
  pre, image      MFMA outputs stored fp32: (4 C + 8) 2^-24 sum |term| + the fragile operands' part; the reference multiplies the
                  same bf16-rounded a and w.  The image adds the library's tanh figure, rtol 1e-6 + atol 1e-7.
  du              stored bf16: 2^-8 |want| + own + flip.  own: 8 * 2^-24 of the magnitudes the fp32 expression is formed from, and
                  the data gradient's own error -- da is rebuilt from (hi, lo) bf16 splits of the gradient image and of w, three
                  MFMAs, 3 * 2^-18 + 52 * 2^-24 of its sum |term|.  flip: the whole term of a fragile ReLU decision.  The reference
                  takes the dgamma / dbeta the kernel's first pass produced (its second pass reads them; checked by themselves).
  fp32 sums       dgamma, dbeta, du_colsum, dw, dbias: 2e-5 sum |term| (every chain is below 300 additions) + own + flip.  dw
                  multiplies bf16(gradient image) with bf16(a): both rounded in the reference, a's fragile part added.
  loss form       the image is bit-equal to the plain forward's; loss (rtol 1e-6), dpre (8 * 2^-24 of its magnitudes) and dbias
                  (2e-5 sum |dpre|) against fp64 ON THE STORED IMAGE, which is checked by itself.
  integer probe   identity BatchNorm, u in {0..3}, integer taps on two channels, dy in {-2..2}: pre EQUALS the integer transposed
                  convolution; dbias, dbeta, dgamma and dw EQUAL the integer sums.  (du_colsum is no integer sum: the backward
                  forms dgamma / dbeta itself, so du is not the masked da.)
Every output is allocated over NaN poison; du and the images are views of buffers with canary rows behind them, which must be
unchanged; two runs give the same bits.

Largest error / bound per class as measured on an MI355X (also DESIGN.md, "Envelope of the fused BatchNorm + conv operators"):
pre / image 0.461 (B=1 H=1025 W=3 C=96 pre); du 0.996 (B=1 H=1025 W=3 C=32: the bf16 store rounding itself); dw 0.410 (B=1 H=1024
W=3 C=128); fp32 sums 0.680 (B=1 H=1 W=1 C=96 du_colsum: one pixel, the sum IS one du); loss 0.045 (B=2 H=5 W=130 C=64 T=260); dpre
0.391 (B=2 H=5 W=130 C=128 T=261).  The integer probes are exact."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, ops  # noqa: E402
from tests.helpers import fused_ref64 as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
BF = torch.bfloat16
WORST = {}
GRAD_SCALE = 0.7
IMG_CANARY_ROWS = 4


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _within(cls, got, want, bound, what):
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an element the kernel did not write?)"
    err = (got.reshape(want.shape) - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[fused output] {what}: error / bound = {ratio:.4f}")
    _note(cls, ratio, what)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _image(B, H, W):
    """An fp32 [B][2H][2W] output over NaN poison with canary rows behind it -> (the view, the whole buffer)."""
    whole = _nan(B * 2 * H + IMG_CANARY_ROWS, 2 * W)
    return whole[:B * 2 * H].view(B, 2 * H, 2 * W), whole


def _intact(whole, rows, what):
    tail = whole[rows:]
    bits = tail.view(torch.int16 if tail.dtype == BF else torch.int32)
    assert bool((bits == (0x7FC0 if tail.dtype == BF else 0x7FC00000)).all()), f"{what}: rows past the end were written"


def _ws(B, H, W, C):
    return ops._ws(torch.device(DEV), "nsg_bn_relu_c1convt_workspace_bytes", B, H, W, C)


def forward(u, mean, invstd, gamma, beta, w, bias, tanh):
    B, H, W, C = u.shape
    y, whole = _image(B, H, W)
    ws, nb = _ws(B, H, W, C)
    p = ops._p
    _lib.call("nsg_bn_relu_c1convt_forward", p(u), ops.NSG_BF16, p(mean), p(invstd), p(gamma), p(beta), p(w), p(bias), p(y),
              ops.NSG_TANH_OUT if tanh else 0, B, H, W, C, p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    _intact(whole, B * 2 * H, "image")
    return y


def forward_mse(u, mean, invstd, gamma, beta, w, bias, target, want_image, want_dbias):
    B, H, W, C = u.shape
    T = target.shape[2]
    (y, y_all), (dpre, dpre_all) = _image(B, H, W), _image(B, H, W)
    loss, dbias = _nan(1), _nan(1)
    ws, nb = _ws(B, H, W, C)
    p = ops._p
    _lib.call("nsg_bn_relu_c1convt_forward_mse", p(u), ops.NSG_BF16, p(mean), p(invstd), p(gamma), p(beta), p(w), p(bias),
              p(y if want_image else None), p(target), T, GRAD_SCALE, p(loss), p(dpre), p(dbias if want_dbias else None), B, H, W, C, p(ws), nb,
              ops._stream())
    torch.cuda.synchronize()
    _intact(y_all, B * 2 * H, "image (loss form)")
    _intact(dpre_all, B * 2 * H, "dpre")
    assert want_image or bool(torch.isnan(y).all()), "the image was written though none was requested"
    assert want_dbias or bool(torch.isnan(dbias).all())
    return loss, dpre, y, dbias


def backward(u, mean, invstd, gamma, beta, w, dy):
    B, H, W, C = u.shape
    M = B * H * W
    whole = torch.full((M + R.OUT_TILE, C), NAN, dtype=BF, device=DEV)
    du = whole[:M]
    cs, dw, dbias, dg, db = _nan(C), _nan(C, 1, 4, 4), _nan(1), _nan(C), _nan(C)
    ws, nb = _ws(B, H, W, C)
    p = ops._p
    _lib.call("nsg_bn_relu_c1convt_backward", p(u), ops.NSG_BF16, p(mean), p(invstd), p(gamma), p(beta), p(w), p(dy), p(du), p(cs), p(dw),
              p(dbias), p(dg), p(db), B, H, W, C, p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    _intact(whole, M, "du")
    return du, cs, dw, dbias, dg, db


def _same(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16) if x.dtype == BF else x, y.view(torch.int16) if y.dtype == BF else y), what


def _dbias_chain(M):
    n4 = 4 * M                              # conv_api.hip cs_geom / colsum_partial_kernel at C = 1: 256 row groups per slab
    n = min(max(R.cdiv(n4, 512), 1), 512)
    return R.cdiv(R.cdiv(n4, n), 256) + 256


def _upload(c):
    c.g = types.SimpleNamespace(**{n: getattr(c, n).to(DEV) for n in ("u", "w", "bias", "gamma", "beta", "dy", "target")})
    c.g.mean, c.g.invstd = ops.bn_stats(c.g.u, c.C)
    c.args = (c.g.u, c.g.mean, c.g.invstd, c.g.gamma, c.g.beta, c.g.w)
    c.ref = (c.u, c.g.mean, c.g.invstd, c.gamma, c.beta, c.w)
    return c


@pytest.fixture(scope="module", params=R.CASES_OUT, ids=lambda p: "B{}-H{}-W{}-C{}".format(*p[0], p[1]))
def case(request):
    return _upload(R.inputs_out(*request.param))


def test_forward(case):
    c = case
    pre = forward(*c.args, c.g.bias, tanh=False)
    _same((pre,), (forward(*c.args, c.g.bias, tanh=False),), "two runs of the forward differ")
    ref = R.output_forward(*c.ref, c.bias)
    bound = R.mfma_bound(ref.pre, ref.terms, ref.frag, ref.K, False)
    _within("pre, image", pre, ref.pre, bound, c.tag + " pre")
    img = forward(*c.args, c.g.bias, tanh=True)
    want = torch.tanh(ref.pre)
    _within("pre, image", img, want, bound + R.TANH_RTOL * want.abs() + R.TANH_ATOL, c.tag + " image")


def test_backward(case):
    c = case
    assert R.out_chain(c.B, c.H, c.W) < R.MAX_CHAIN and R.out_dw_chain(c.B, c.H, c.W) < R.MAX_CHAIN and _dbias_chain(c.M) < R.MAX_CHAIN
    out = backward(*c.args, c.g.dy)
    _same(out, backward(*c.args, c.g.dy), "two runs of the backward differ")
    du, cs, dw, dbias, dg, db = out
    o = R.output_backward(*c.ref, c.dy, dgamma_used=dg, dbeta_used=db)
    k = R.SUM_COEF
    _within("fp32 sums", dg, o.dgamma, k * o.dgamma_terms + o.dgamma_own + o.dgamma_flip, c.tag + " dgamma")
    _within("fp32 sums", db, o.dbeta, k * o.dbeta_terms + o.dbeta_own + o.dbeta_flip, c.tag + " dbeta")
    _within("du", du, o.du, R.UB * o.du.abs() + o.du_own + o.du_flip, c.tag + " du")
    _within("fp32 sums", cs, o.du_colsum, k * o.du_colsum_terms + o.du_colsum_own + o.du_colsum_flip, c.tag + " du_colsum")
    _within("dw", dw, o.dw, k * o.dw_terms + o.dw_frag, c.tag + " dw")
    _within("fp32 sums", dbias[0], o.dbias, k * o.dbias_terms, c.tag + " dbias")


MSE_CASES = [(s, C, e) for s, C in R.CASES_OUT if s in R.MSE_SHAPES for e in R.MSE_EXTRA]


@pytest.mark.parametrize("shape,C,extra", MSE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_form(shape, C, extra):
    c = _upload(R.inputs_out(shape, C))
    T = 2 * c.W + extra
    target = c.target[:, :, :T].contiguous()
    tg = target.to(DEV)
    img = forward(*c.args, c.g.bias, tanh=True)
    loss, dpre, y, _ = forward_mse(*c.args, c.g.bias, tg, True, False)
    _same((y,), (img,), "the loss form stores another image than the plain forward")
    loss2, dpre2, _, dbias = forward_mse(*c.args, c.g.bias, tg, False, True)
    _same((loss2, dpre2), (loss, dpre), "the loss form's two variants differ")
    l64, dpre64, mag, db64, sum_abs = R.mse_epilogue(img.cpu(), target, GRAD_SCALE)
    tag = f"{c.tag} T={T}"
    _within("loss", loss[0], l64, 1e-6 * l64.abs(), tag + " loss")
    _within("dpre", dpre, dpre64, R.WINDOW * mag, tag + " dpre")
    _within("fp32 sums", dbias[0], dpre.double().sum().cpu(), R.SUM_COEF * sum_abs, tag + " dbias (loss form)")


@pytest.mark.parametrize("shape,C", R.PROBE_OUT, ids=lambda v: str(v).replace(" ", ""))
def test_integer_probe(shape, C):
    p = R.probe_out(shape, C)
    u, w, dy, zero, one = (t.to(DEV) for t in (p.u, p.w, p.dy, p.zero, p.one))
    bias = torch.tensor([2.0])
    args = (u, zero, one, one, zero, w)
    ref = R.output_forward(p.u, p.zero, p.one, p.one, p.zero, p.w, bias)
    exact = lambda got, want, what: torch.testing.assert_close(got.double().cpu().reshape(want.shape), want, rtol=0, atol=0,  # noqa: E731
                                                               msg=lambda m: f"{p.tag} {what}: {m}")
    exact(forward(*args, bias.to(DEV), tanh=False), ref.pre, "pre")
    du, cs, dw, dbias, dg, db = backward(*args, dy)
    o = R.output_backward(p.u, p.zero, p.one, p.one, p.zero, p.w, p.dy)
    exact(dbias[0], o.dbias, "dbias")
    exact(db, o.dbeta, "dbeta")
    exact(dg, o.dgamma, "dgamma")
    exact(dw, o.dw, "dw")
    assert bool(torch.isfinite(du.float()).all()) and bool(torch.isfinite(cs).all())


def test_rejections_launch_nothing():
    def raw_forward(u, C, y, dims, dtype=BF, ws_short=0):
        B, H, W = dims
        v, w = torch.ones(max(C, 1), device=DEV), torch.zeros(max(C, 1), 16, device=DEV)
        ws, nb = _ws(max(B, 1), max(H, 1), max(W, 1), C if ops.bn_relu_c1convt_supported(BF, C) else 128)
        p = ops._p
        _lib.call("nsg_bn_relu_c1convt_forward", p(u), ops.nsg_dtype(dtype), p(v), p(v), p(v), p(v), p(w), p(None), p(y), 0, B, H, W, C, p(ws),
                  nb - ws_short, ops._stream())

    def refused(fn, *outs):
        with pytest.raises(_lib.NsgError):
            fn()
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o.float()).all()), "a refused call wrote to its output"

    B, H, W = 2, 3, 5
    y = _nan(B, 2 * H, 2 * W)
    for C in (160, 16):
        assert not ops.bn_relu_c1convt_supported(BF, C)
        u = torch.ones(B, H, W, C, dtype=BF, device=DEV)
        refused(lambda: raw_forward(u, C, y, (B, H, W)), y)
    C = 64
    u = torch.ones(B, H, W, C, dtype=BF, device=DEV)
    assert not ops.bn_relu_c1convt_supported(torch.float32, C)
    refused(lambda: raw_forward(u.float(), C, y, (B, H, W), dtype=torch.float32), y)
    for dims in ((0, H, W), (B, 0, W), (B, H, 0)):
        refused(lambda: raw_forward(u, C, y, dims), y)
    refused(lambda: raw_forward(u, C, y, (B, H, W), ws_short=1), y)
    # the loss form: a target narrower than the image; the backward: a short workspace
    v, w = torch.ones(C, device=DEV), torch.zeros(C, 16, device=DEV)
    ws, nb = _ws(B, H, W, C)
    p = ops._p
    loss, dpre = _nan(1), _nan(B, 2 * H, 2 * W)
    tg = torch.zeros(B, 2 * H, 2 * W - 1, device=DEV)
    refused(lambda: _lib.call("nsg_bn_relu_c1convt_forward_mse", p(u), ops.NSG_BF16, p(v), p(v), p(v), p(v), p(w), p(None), p(None), p(tg), 2 * W - 1,
                              1.0, p(loss), p(dpre), p(None), B, H, W, C, p(ws), nb, ops._stream()), loss, dpre)
    tg = torch.zeros(B, 2 * H, 2 * W, device=DEV)
    refused(lambda: _lib.call("nsg_bn_relu_c1convt_forward_mse", p(u), ops.NSG_BF16, p(v), p(v), p(v), p(v), p(w), p(None), p(None), p(tg), 2 * W,
                              1.0, p(loss), p(dpre), p(None), B, H, W, C, p(ws), nb - 1, ops._stream()), loss, dpre)
    du, dw, dg, db = torch.full((B * H * W, C), NAN, dtype=BF, device=DEV), _nan(C, 16), _nan(C), _nan(C)
    dy = torch.zeros(B, 2 * H, 2 * W, device=DEV)
    refused(lambda: _lib.call("nsg_bn_relu_c1convt_backward", p(u), ops.NSG_BF16, p(v), p(v), p(v), p(v), p(w), p(dy), p(du), p(None), p(dw), p(None),
                              p(dg), p(db), B, H, W, C, p(ws), nb - 1, ops._stream()), du, dw, dg, db)


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[fused output summary] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
