"""GPU tests of the latent prior at its production width: GatedPixelCNN(512, 64, 15) on a B x 20 x 256 code grid (DESIGN.md
section 5b).  Every kernel the prior runs is compared with an fp64 evaluation of the same operation on the same fp32
operands (ATen in float64, or oracle/pixelcnn_oracle.py on a state dict converted to double): the conv layer set of the
masked stacks and the output stack, the gated activation with its conditioning rows, the two embeddings, the
cross-entropy over a matrix of logit regimes; then the whole model against the fp64 oracle, and the exact properties of
the timed shape (64 clips): batch independence, causality, the loss as a mean of per-clip losses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from oracle import pixelcnn_oracle as P  # noqa: E402
from tests.helpers.prior_ref import _ce64  # noqa: E402,F401

DEV = "cuda:0"
INPUT_DIM, DIM, N_LAYERS, N_CLASSES = 512, 64, 15, 10


def gpu(t):
    return t.to(DEV).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _close(got, want, tol=2e-5, what=""):
    """The suite's convention (tests/test_gpu_ops.py): max abs error within tol of the reference's max |value|."""
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got.double() - want.double()).abs().max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. the prior's conv layer set (fp32, gather_gemm / wgrad_gemm) against fp64 F.conv2d + crop and its autograd
# ---------------------------------------------------------------------------------------------
PRIOR_LAYERS = [
    # (name, C_in, C_out, (kh, kw), (ph, pw), mask): mask zeroes the last kernel row ("row") or column ("col") as make_causal does
    ("vert7", 64, 128, (4, 7), (3, 3), None),
    ("vert7_causal", 64, 128, (4, 7), (3, 3), "row"),
    ("vert3", 64, 128, (2, 3), (1, 1), None),
    ("horiz7", 64, 128, (1, 4), (0, 3), None),
    ("horiz7_causal", 64, 128, (1, 4), (0, 3), "col"),
    ("horiz3", 64, 128, (1, 2), (0, 1), None),
    ("v2h_1x1", 128, 128, (1, 1), (0, 0), None),
    ("resid_1x1", 64, 64, (1, 1), (0, 0), None),
    ("out0_1x1", 64, 512, (1, 1), (0, 0), None),
    ("out2_1x1", 512, 512, (1, 1), (0, 0), None),
]
PRIOR_GRIDS = [(2, 20, 256), (3, 20, 37), (2, 1, 37), (2, 20, 1), (1, 1, 1)]


@pytest.mark.parametrize("grid", PRIOR_GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("layer", PRIOR_LAYERS, ids=lambda c: c[0])
def test_prior_conv_layer_set(layer, grid):
    """Forward (plain and with the fused ReLU store), data gradient, weight and bias gradient of each conv the prior runs at
    width 64, on the latent grid, a ragged width and the degenerate extents where the padding and the crop cover almost every
    tap.  Within 2e-5 of the fp64 result's max |value|; the weight gradient bitwise reproducible."""
    name, Ci, Co, (kh, kw), (ph, pw), mask = layer
    B, H, W = grid
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + B * 97 + H * 7 + W)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, kh, kw, generator=g) * (1.0 / (Ci * kh * kw) ** 0.5)
    if mask == "row":
        w[:, :, -1].zero_()
    elif mask == "col":
        w[:, :, :, -1].zero_()
    b = torch.randn(Co, generator=g) * 0.1
    dy = torch.randn(B, Co, H, W, generator=g)

    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv2d(x64, w64, b64, 1, (ph, pw))[:, :, :H, :W]
    assert tuple(y64.shape) == (B, Co, H, W)
    gx, gw, gb = torch.autograd.grad(y64, [x64, w64, b64], dy.double())
    y64 = y64.detach()

    d = ops.conv_desc(B, H, W, Ci, Co, (kh, kw), 1, (ph, pw), out_hw=(H, W))
    wf, wd = ops.pack_weights(d, gpu(w))
    xg, dyg, bg = gpu(nhwc(x)), gpu(nhwc(dy)), gpu(b)
    _close(nchw(ops.conv_forward(d, xg, wf, bg).cpu()), y64, what="forward")
    _close(nchw(ops.conv_forward(d, xg, wf, bg, flags=ops.NSG_RELU_OUT).cpu()), torch.relu(y64), what="forward + ReLU")
    _close(nchw(ops.conv_dgrad(d, dyg, wd).cpu()), gx, what="dgrad")
    dwg, dbg = ops.conv_wgrad(d, xg, dyg, tuple(w.shape))
    _close(dwg.cpu(), gw, what="wgrad")
    _close(dbg.cpu(), gb, what="bias grad")
    dwg2, dbg2 = ops.conv_wgrad(d, xg, dyg, tuple(w.shape))
    assert torch.equal(dwg, dwg2) and torch.equal(dbg, dbg2), "wgrad must be bitwise reproducible"


# ---------------------------------------------------------------------------------------------
# 2. gated activation, the class-conditioning sum, the two embeddings
# ---------------------------------------------------------------------------------------------
def _gate64(x, cond, dy):
    """fp64 tanh(a) * sigmoid(b) of the channel halves of x + cond (per clip), and its gradients w.r.t. x and cond."""
    B = cond.shape[0]
    x64 = x.double().requires_grad_(True)
    c64 = cond.double().requires_grad_(True)
    z = x64.view(B, -1, x.shape[-1]) + c64[:, None, :]
    a, b = z.chunk(2, dim=-1)
    y = torch.tanh(a) * torch.sigmoid(b)
    gx, gc = torch.autograd.grad(y, [x64, c64], dy.double().view(y.shape))
    return y.detach().view(*x.shape[:-1], -1), gx, gc


@pytest.mark.parametrize("regime", ["randn", "saturating"])
def test_prior_gated_activation_at_width(regime):
    """M = 2 x 20 x 256 rows of C = 64 (the gate of every layer), one conditioning row per clip.  Saturating: |a| up to 30,
    b in +-100 (expf(-b) overflows to inf): the outputs stay finite and within 1e-6 absolute of fp64."""
    B, H, W, C = 2, 20, 256, 64
    g = torch.Generator().manual_seed(11 if regime == "randn" else 12)
    if regime == "randn":
        x = torch.randn(B, H, W, 2 * C, generator=g) * 2
        cond = torch.randn(B, 2 * C, generator=g)
    else:
        a = (torch.rand(B, H, W, C, generator=g) * 2 - 1) * 28
        b = (torch.rand(B, H, W, C, generator=g) * 2 - 1) * 98
        a.view(-1)[:4] = torch.tensor([28.0, -28.0, 0.0, 1e-3])
        b.view(-1)[:4] = torch.tensor([98.0, -98.0, -98.0, 98.0])
        x = torch.cat([a, b], dim=-1)
        cond = torch.cat([torch.tensor([[2.0] * C + [2.0] * C], dtype=torch.float32),
                          torch.tensor([[-2.0] * C + [-2.0] * C], dtype=torch.float32)])   # reaches |a| = 30, |b| = 100
    dy = torch.randn(B, H, W, C, generator=g) if regime == "randn" else torch.rand(B, H, W, C, generator=g) * 2 - 1
    y64, gx64, gc64 = _gate64(x, cond, dy)
    xg, cg, dyg = gpu(x), gpu(cond), gpu(dy)
    y = ops.gated_activation(xg, cg)
    dx = ops.gated_activation_backward(xg, cg, dyg)
    dc = ops.clip_colsum(dx, B)
    for t, nm in ((y, "y"), (dx, "dx"), (dc, "dcond")):
        assert bool(torch.isfinite(t).all()), f"{nm}: non-finite values"
    if regime == "randn":
        _close(y.cpu(), y64, what="gated forward")
        _close(dx.cpu(), gx64, what="gated backward")
    else:
        assert float((y.cpu().double() - y64).abs().max()) <= 1e-6, "gated forward (saturating)"
        assert float((dx.cpu().double() - gx64).abs().max()) <= 1e-6, "gated backward (saturating)"
    # the conditioning gradient: clip_colsum of the kernel's own dx against its fp64 sum, and against the fp64 autograd
    _close(dc.cpu(), dx.cpu().double().view(B, -1, 2 * C).sum(1), tol=1e-5, what="clip_colsum vs fp64 sum")
    _close(dc.cpu(), gc64, what="conditioning gradient")


@pytest.mark.parametrize("impl", ["f32", "sorted"])
@pytest.mark.parametrize("K,D,N", [(512, 64, 64 * 20 * 256), (10, 128, 2), (10, 128, 64)], ids=["codes", "classes_b2", "classes_b64"])
def test_prior_embeddings_at_width(K, D, N, impl):
    """gather_rows (bitwise: a copy) and index_add_rows against fp64 index_add at the prior's two embedding tables: the 512 x 64
    code table with 327 680 indices (the timed shape) and the 10 x 128 class table with one label per clip."""
    g = torch.Generator().manual_seed(K * 1000 + N)
    table = torch.randn(K, D, generator=g)
    idx = torch.randint(0, K, (N,), generator=g)
    got = ops.gather_rows(gpu(table), gpu(idx))
    assert torch.equal(got.cpu(), table[idx])
    v = torch.randn(N, D, generator=g)
    want = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, v.double())
    out = ops.index_add_rows(gpu(idx), gpu(v), K, impl=impl)
    assert torch.equal(out, ops.index_add_rows(gpu(idx), gpu(v), K, impl=impl)), "index_add_rows must be bitwise reproducible"
    scale = float(want.abs().max())
    np.testing.assert_allclose(out.cpu().double().numpy(), want.numpy(), rtol=1e-5, atol=2e-6 * scale + 1e-6)


# ---------------------------------------------------------------------------------------------
# 3. cross-entropy against fp64 over a matrix of logit regimes
# ---------------------------------------------------------------------------------------------
CE_REGIMES = ["randn", "offset+100", "offset+300", "offset-300", "confident", "confident_offset+50", "tied", "constant"]
CE_SHAPES = [(M, K) for M in (1, 3, 4, 5, 2047) for K in (1, 2, 63, 64, 65, 512)] + [(327680, 512)]


def _ce_logits(regime, M, K, gen):
    """(M, K) fp32 logits and int64 targets on the GPU for one regime."""
    l = torch.randn(M, K, device=DEV, generator=gen)
    t = torch.randint(0, K, (M,), device=DEV, generator=gen)
    rows = torch.arange(M, device=DEV)
    if regime.startswith("offset"):
        l += float(regime[len("offset"):])
    elif regime.startswith("confident"):
        # the target 12 to 30 above the largest of the rest
        lift = 12 + 18 * torch.rand(M, device=DEV, generator=gen)
        l[rows, t] = l.amax(dim=1) + lift
        if "offset" in regime:
            l += float(regime.split("offset")[1])
    elif regime == "tied":
        # two entries share the row's maximum; in every other row one of them is the target
        other = torch.randint(0, K, (M,), device=DEV, generator=gen)
        first = torch.where(rows % 2 == 0, t, torch.randint(0, K, (M,), device=DEV, generator=gen))
        top = l.amax(dim=1) + 1
        l[rows, first] = top
        l[rows, other] = top
    elif regime == "constant":
        l = (torch.randn(M, 1, device=DEV, generator=gen) * 50).expand(M, K).contiguous()
    return l.contiguous(), t


def _ce_check(l, t, grad_scale, what):
    loss, dl = ops.cross_entropy(l, t, grad_scale=grad_scale)
    want, g64 = _ce64(l, t, grad_scale)
    # the closed form is the ATen op: fp64 F.cross_entropy and its autograd agree with it to their own rounding
    l64 = l.double().requires_grad_(True)
    aten = F.cross_entropy(l64, t)
    (g_aten,) = torch.autograd.grad(aten * grad_scale, [l64])
    aten = aten.detach()
    M = l.shape[0]
    assert abs(float(aten) - float(want)) <= 1e-12 * (1.0 + float(l.abs().max())), f"{what}: fp64 reference vs F.cross_entropy"
    assert float((g_aten - g64).abs().max()) <= 1e-12 * (1.0 + float(l.abs().max())) * grad_scale / M, f"{what}: fp64 gradient vs autograd"
    got, want = float(loss.item()), float(want.item())
    assert abs(got - want) <= 1e-6 * abs(want), f"{what}: mean loss {got!r} vs fp64 {want!r} (rel {abs(got - want) / max(abs(want), 1e-300):.2e})"
    err = (dl.double() - g64).abs().amax(dim=1)
    bound = 1e-5 * g64.abs().amax(dim=1)
    bad = int((err > bound).sum())
    if bad:
        r = int(torch.argmax(err - bound))
        raise AssertionError(f"{what}: {bad} rows' gradients beyond 1e-5 of the row scale; row {r}: err {float(err[r]):.3e}, "
                             f"scale {float(g64[r].abs().max()):.3e}")


@pytest.mark.parametrize("regime", CE_REGIMES)
def test_prior_cross_entropy_regimes(regime):
    """Mean loss within 1e-6 relative of fp64, every row's gradient within 1e-5 of that row's largest |fp64| entry, at
    M in {1, 3, 4, 5, 2047, 327 680} and K in {1, 2, 63, 64, 65, 512}, grad_scale 1 and 0.37.  fp32 ATen itself misses these
    bounds on the confident and offset rows, so the reference is fp64 (_ce64, held to fp64 F.cross_entropy)."""
    gen = torch.Generator(device=DEV).manual_seed(CE_REGIMES.index(regime) + 1)
    for M, K in CE_SHAPES:
        l, t = _ce_logits(regime, M, K, gen)
        for gs in (1.0, 0.37):
            _ce_check(l, t, gs, f"{regime} M={M} K={K} grad_scale={gs}")
        if M == 327680:   # deterministic: the fixed-order reduction of the mean
            a, da = ops.cross_entropy(l, t)
            b, db = ops.cross_entropy(l, t)
            assert torch.equal(a, b) and torch.equal(da, db)


# ---------------------------------------------------------------------------------------------
# 4. the module at production width against the fp64 oracle
# ---------------------------------------------------------------------------------------------
def _rel_l2(a, truth):
    return (a.double() - truth).norm().item() / max(truth.norm().item(), 1e-30)


def _model(bias_offset=0.0):
    torch.manual_seed(1)
    m = GatedPixelCNN(INPUT_DIM, DIM, N_LAYERS, N_CLASSES)
    if bias_offset:
        with torch.no_grad():
            m.output_conv[2].bias += bias_offset
    return m


def _gpu_loss_and_grads(st, x, label):
    m = GatedPixelCNN(INPUT_DIM, DIM, N_LAYERS, N_CLASSES)
    m.load_state_dict(st)
    m = m.to(DEV)
    logits = m(gpu(x), gpu(label))
    loss = m.loss(gpu(x), gpu(label))
    loss.backward()
    return logits.detach().cpu(), loss.detach().cpu(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("W,bias_offset", [(256, 0.0), (37, 0.0), (256, 200.0)], ids=["20x256", "20x37", "20x256_bias+200"])
def test_prior_production_width_against_oracle(W, bias_offset):
    """GatedPixelCNN(512, 64, 15, 10) at seed 1, B = 2: logits within 1e-5 of their scale, the loss within 1e-6 relative and
    each parameter gradient within max(4 x the fp32 CPU oracle's own distance, 1e-5) relative L2 of the fp64 oracle on the
    same state (make_causal zeroes layer 0's masked taps in place on both sides).  The +200 bias variant puts the
    cross-entropy on offset logits.  Two runs give bitwise identical gradients."""
    torch.set_num_threads(16)
    B, H = 2, 20
    st = {k: v.clone() for k, v in _model(bias_offset).state_dict().items()}
    g = torch.Generator().manual_seed(W)
    x = torch.randint(0, INPUT_DIM, (B, H, W), generator=g)
    label = torch.randint(0, N_CLASSES, (B,), generator=g)
    logits32, loss32, grads32, _ = P.loss_and_grads({k: v.clone() for k, v in st.items()}, x, label, N_LAYERS)
    logits64, loss64, grads64, _ = P.loss_and_grads({k: v.double() for k, v in st.items()}, x, label, N_LAYERS)

    logits, loss, grads = _gpu_loss_and_grads(st, x, label)
    _close(logits, logits64, tol=1e-5, what="logits")
    assert abs(loss.item() - loss64.item()) <= 1e-6 * abs(loss64.item()), f"loss {loss.item()!r} vs fp64 {loss64.item()!r}"
    assert len(grads) == len(grads64)
    for k, gk in grads.items():
        err_gpu = _rel_l2(gk.cpu(), grads64[k])
        err_cpu = _rel_l2(grads32[k], grads64[k])
        assert err_gpu <= max(4.0 * err_cpu, 1e-5), f"{k}: GPU {err_gpu:.2e} vs CPU-fp32 {err_cpu:.2e} (relative L2 to fp64)"
    _, _, grads2 = _gpu_loss_and_grads(st, x, label)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), f"{k}: gradients differ between two identical runs"


# ---------------------------------------------------------------------------------------------
# 5. full-size properties at the timed shape, 64 x 20 x 256 (no BatchNorm: each is exact)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_size():
    B, H, W = 64, 20, 256
    model = _model().to(DEV)
    g = torch.Generator().manual_seed(64)
    x = gpu(torch.randint(0, INPUT_DIM, (B, H, W), generator=g))
    label = gpu(torch.randint(0, N_CLASSES, (B,), generator=g))
    with torch.no_grad():
        logits = model.forward_nhwc(x, label)
    return model, x, label, logits


def test_prior_full_size_batch_independence(full_size):
    model, x, label, logits = full_size
    with torch.no_grad():
        for c in (0, 31, 63):
            alone = model.forward_nhwc(x[c:c + 1], label[c:c + 1])
            assert torch.equal(alone, logits[c:c + 1]), f"clip {c}: logits in the batch differ from the clip run alone"


CAUSAL_POSITIONS = [(0, 0), (0, 255), (7, 100), (19, 255)]


def test_prior_full_size_causality(full_size):
    """Each position's logits depend only on the codes before it in raster order: replacing the codes at p and at every later
    position leaves the logits of every position up to and including p bitwise unchanged, and changes some later one."""
    model, x, label, logits = full_size
    B, H, W = x.shape
    x2 = x.clone()
    g = torch.Generator().manual_seed(5)
    clips = [3, 20, 41, 63]
    for c, (i, j) in zip(clips, CAUSAL_POSITIONS):
        p = i * W + j
        flat = x2[c].view(-1)
        flat[p:] = (flat[p:] + gpu(torch.randint(1, INPUT_DIM, (H * W - p,), generator=g))) % INPUT_DIM
    with torch.no_grad():
        logits2 = model.forward_nhwc(x2, label)
    for c, (i, j) in zip(clips, CAUSAL_POSITIONS):
        p = i * W + j
        a, b = logits[c].reshape(H * W, -1), logits2[c].reshape(H * W, -1)
        assert torch.equal(a[:p + 1], b[:p + 1]), f"clip {c}: logits at or before {(i, j)} changed"
        if p + 1 < H * W:
            assert not torch.equal(a[p + 1:], b[p + 1:]), f"clip {c}: no later logits changed (the check would be vacuous)"
    untouched = [c for c in range(B) if c not in clips]
    assert torch.equal(logits[untouched], logits2[untouched])


def test_prior_full_size_loss_is_the_mean_of_clip_losses(full_size):
    model, x, label, _ = full_size
    with torch.no_grad():
        batch = float(model.loss(x, label).item())
        per_clip = [float(model.loss(x[c:c + 1], label[c:c + 1]).item()) for c in range(x.shape[0])]
    want = float(np.mean(np.array(per_clip, dtype=np.float64)))
    assert abs(batch - want) <= 1e-6 * abs(want), f"batch loss {batch!r} vs the mean of the clips' {want!r}"
