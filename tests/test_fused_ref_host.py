"""tests/helpers/fused_ref64.py on the CPU: (1) every function agrees with torch.autograd in fp64 on the same composition when no
bf16 rounding is applied; (2) the case tables of tests/test_gpu_fused_1x1_envelope.py and tests/test_gpu_fused_output_envelope.py
sit on the kernels' geometry as listed here -- a later change of a tile size fails HERE, it does not silently move an edge; (3) for
every case the reference alone keeps the conditions the bounds rest on: the share of fragile elements of every rounded intermediate
is at most 1e-3, the fragile terms make up more than half of a bound for at most 1 % of the outputs, every fp32 chain is stated
(below 300 additions, or its bound's coefficient is the chain's own), and the integer probes are exact in fp32 (operands exact in
bf16, every sum of magnitudes below 2^24).

Exempt, with their reason: (a) the single row, M = 1, from the share and the half-of-the-bound conditions.  Batch statistics of one
row are mean = x and invstd = 1 / sqrt(eps) = 316: a = relu(beta + 0 * 316 gamma) is formed from magnitudes a thousand times its
value, so the window covers a quarter of a bf16 step whatever the seed, and the BatchNorm backward of one row is identically zero:
dh is the fp32 rounding residue and the bound of dx is that residue alone.  The bounds still hold there (the fragile terms are in
them); what M = 1 shows sharply is the integer probe, whose identity statistics have no such magnitudes.  (b) Outputs whose fp64
value is itself below their fragile term: a dot product that cancels to one operand's bf16 ulp has no tighter bound.  (c) The
weight gradients below 4096 rows.  A dw entry is an fp32 sum of M products, held to 2e-5 sum |term|; ONE fragile operand among its
2 M moves it by a bf16 ulp, 2^-8 of a term, which is the whole of such a bound up to M = 200 and half of it up to a few thousand:
one entry in ten holds one at M = 128.  No seed changes that.  At those sizes the weight gradient's exactness is the integer
probe's to show, and the condition is asserted from 4096 rows on."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import bn_ref64 as BN
from tests.helpers import fused_ref64 as R

EPS = BN.EPS
SHARE = 1e-3
BIG = 20000                 # rows from which the host checks count on the inputs and the staged operands only (no fp64 GEMMs)


def _close(got, want, what):
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13, msg=lambda m: f"{what}: {m}")


def _bn_eval(x, mean, invstd, gamma, beta):
    """F.batch_norm with GIVEN statistics (NCHW or [M][C] input)."""
    return F.batch_norm(x, mean, 1.0 / invstd ** 2 - EPS, gamma, beta, False, 0.0, EPS)


# ----------------------------------------------------------------------------------------------------------------------
# (1) the yardstick against autograd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(1, 8), (5, 8), (13, 16)])
def test_conv1x1_reference_is_autograd(M, C):
    g = torch.Generator().manual_seed(M + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x, dy = rnd(M, C) * 1.3 + 0.4, rnd(M, C)
    w, bias = (rnd(C, C) * 0.3).requires_grad_(True), rnd(C).requires_grad_(True)
    mean, invstd = rnd(C) * 0.2, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma, beta = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True), (rnd(C) * 0.3).requires_grad_(True)
    gamma2, beta2 = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, rnd(C)
    a = F.relu(_bn_eval(x, mean, invstd, gamma, beta))
    a.retain_grad()
    h = F.conv2d(a.t().reshape(1, C, M, 1), w.reshape(C, C, 1, 1), bias)[0, :, :, 0].t()
    h.retain_grad()
    fwd = R.conv1x1_forward(x, mean, invstd, gamma, beta, w, bias, round_ops=False)
    _close(fwd.y, h.detach(), "y")
    assert not bool(fwd.frag.any())
    if M == 1:
        return          # ATen refuses a training-mode BatchNorm over one value per channel; BN.backward covers M = 1 in test_bn_ref_host.py
    F.batch_norm(h, None, None, gamma2, beta2, True, 0.1, EPS).mul(dy).sum().backward()
    m2, i2, _ = BN.stats(h.detach())
    _, dg2, db2, _ = BN.backward(h.detach(), dy, m2, i2, gamma2)
    bwd = R.conv1x1_backward(h.detach(), dy, m2, i2, gamma2, dg2, db2, w.detach(), round_ops=False)
    _close(bwd.dh, h.grad, "dh")
    _close(bwd.dx, a.grad, "dx")
    _close(bwd.colsum, bias.grad, "dh_colsum")
    ps = R.prev_sums(x, bwd.dx, mean, invstd, gamma.detach(), beta.detach())
    _close(ps.dgamma, gamma.grad, "prev_dgamma")
    _close(ps.dbeta, beta.grad, "prev_dbeta")
    act = R.staged_activation(x, mean, invstd, gamma, beta, round_ops=False)
    dw, terms, frag = R.conv1x1_wgrad(bwd.dh_r, bwd.dh_delta, act)
    _close(dw, w.grad, "dw")
    assert bool((terms >= dw.abs() - 1e-12).all()) and not bool(frag.any())


@pytest.mark.parametrize("B,H,W,C,extra", [(1, 1, 1, 8, 0), (2, 3, 2, 8, 1), (1, 2, 5, 16, 4)])
def test_output_layer_reference_is_autograd(B, H, W, C, extra):
    g = torch.Generator().manual_seed(B + H + W + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    u = rnd(B, H, W, C) * 1.5 + 0.5
    w = (rnd(C, 1, 4, 4) * 0.2).requires_grad_(True)
    bias = (rnd(1) * 0.1).requires_grad_(True)
    gamma, beta = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True), (rnd(C) * 0.3).requires_grad_(True)
    dy = rnd(B, 2 * H, 2 * W)
    un = u.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    # forward with given statistics, and the loss epilogue
    mean, invstd = rnd(C) * 0.2, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    pre = F.conv_transpose2d(F.relu(_bn_eval(un, mean, invstd, gamma, beta)), w, bias, 2, 1)[:, 0]
    fwd = R.output_forward(u, mean, invstd, gamma, beta, w, bias, round_ops=False)
    _close(fwd.pre, pre.detach(), "pre")
    T = 2 * W + extra
    target = torch.rand(B, 2 * H, T, generator=g, dtype=torch.float64)
    img = torch.tanh(pre.detach()).requires_grad_(True)
    loss = F.mse_loss(F.pad(img, (0, extra)), target)
    (gi,) = torch.autograd.grad(loss, img)
    l64, dpre, mag, dbias, _ = R.mse_epilogue(img.detach(), target, 0.7)
    _close(l64, loss.detach(), "loss")
    _close(dpre, 0.7 * gi * (1.0 - img.detach() ** 2), "dpre")
    _close(dbias, dpre.sum(), "dbias of the loss form")
    assert bool((mag >= dpre.abs() - 1e-15).all())
    if B * H * W == 1:
        return
    # backward of the chain with batch statistics
    F.conv_transpose2d(F.relu(F.batch_norm(un, None, None, gamma, beta, True, 0.1, EPS)), w, bias, 2, 1)[:, 0].mul(dy).sum().backward()
    m, i, _ = BN.stats(u.reshape(-1, C))
    o = R.output_backward(u, m, i, gamma.detach(), beta.detach(), w.detach(), dy, round_ops=False)
    _close(o.du, un.grad.permute(0, 2, 3, 1).reshape(-1, C), "du")
    _close(o.dw, w.grad.reshape(C, 16), "dw")
    _close(o.dbias, bias.grad[0], "dbias")
    _close(o.dgamma, gamma.grad, "dgamma")
    _close(o.dbeta, beta.grad, "dbeta")
    _close(o.du_colsum, un.grad.sum((0, 2, 3)), "du_colsum")


def test_rounding_helpers():
    v = torch.tensor([1.0, 1.00390625, 1.0039, 0.0, -3.0, 2.0 ** -20], dtype=torch.float64)
    assert R.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -6, 2.0 ** -27]
    r, delta, frag, noise = R.round_fragile(v, torch.ones_like(v))
    assert frag.tolist() == [False, True, False, False, False, False]      # 1 + 2^-8 is the midpoint between 1 and 1 + 2^-7
    assert noise.tolist() == [False, False, False, True, False, False] or noise.tolist() == [False, False, False, True, False, True]
    assert float(delta[1]) == 2.0 ** -7 + 2.0 * R.WINDOW and float(delta[0]) == 0.0
    assert R.WINDOW_A == 4 * R.U32 and R.WINDOW == 8 * R.U32
    assert R.rb(v).tolist()[:3] == [1.0, 1.0, 1.0078125] or R.rb(v).tolist()[:3] == [1.0, 1.0, 1.0]


# ----------------------------------------------------------------------------------------------------------------------
# (2) the case tables against the geometry
# ----------------------------------------------------------------------------------------------------------------------
def test_case_tables_sit_on_the_kernel_geometry():
    # gemm_flat.hip: ROWS = 128, FLAT_BLOCKS = 512; WROWS = 64, FLAT_WIDE_BLOCKS = 256; FLAT_FUSED_BLOCKS = 256.  gemm_wgrad.hip
    # plan_slabs: slabs of at least 256 rows, one round of 512 blocks over the tiles.  c1_mfma.hip / conv_api.hip: 128-row blocks
    # of the dots kernel capped at 1024 (512 at C = 256), 64-pixel tiles capped at NSG_MAX_SLABS = 1024.
    assert R.boundary_ms(128) == R.boundary_ms(32) == R.boundary_ms(64) == [1, 31, 127, 128, 129, 256, 257, 65536, 65537]
    assert R.boundary_ms(256) == [1, 31, 63, 64, 65, 256, 257, 16384, 16385]
    assert (R.FUSED_BLOCKS * R.FUSED_ROWS, R.RAGGED_M) == (32768, 196685)
    assert (R.wgrad_cap_m(128), R.wgrad_cap_m(256)) == (130817, 32513)
    for C in (32, 64, 128, 256):
        cap = R.wgrad_cap_m(C)
        assert R.wgrad_slabs(256, C)[0] == 1 and R.wgrad_slabs(257, C)[0] == 2, "the weight gradient's first slab split moved"
        assert R.wgrad_slabs(cap, C)[0] == R.wgrad_slabs(10 * cap, C)[0] > R.wgrad_slabs(cap - 1, C)[0], "its slab cap moved"
    ms = {C: [m for m, c in R.CASES_1X1 if c == C] for C in (32, 64, 128, 256)}
    assert set(R.boundary_ms(128) + [32768, 32769, 130817, 196685]) == set(ms[128])
    assert set(R.boundary_ms(256) + [32513]) == set(ms[256]) and set(R.boundary_ms(32)) == set(ms[32]) and ms[64] == [1, 129, 65537]
    for M, C in R.CASES_1X1:        # the tile a persistent block takes: one up to the cap, a second one right behind it
        rows, blocks, per_block, _, _ = R.flat_geom(M, C)
        assert per_block == R.cdiv(R.cdiv(M, rows), blocks)
    assert R.flat_geom(65536, 128)[2] == 1 and R.flat_geom(65537, 128)[2] == 2 and R.flat_geom(196685, 128)[2] == 4
    assert R.flat_geom(16384, 256)[2] == 1 and R.flat_geom(16385, 256)[2] == 2
    assert R.fused_geom(32768) == (256, 1) and R.fused_geom(32769) == (256, 2)
    # the output layer
    assert R.TILE_EDGE == [(1, 1, 63), (1, 1, 64), (1, 1, 65)]
    assert [R.out_tiles(*s) for s in R.BWD_CAP] == [1024, 1025, 1025] and R.BWD_CAP[2] == (5, 205, 1)
    assert R.fwd_cap(128) == [(1, 2048, 64), (1, 131073, 1)] and R.fwd_cap(256) == [(1, 1024, 64), (1, 65537, 1)]
    assert [b * h * w for b, h, w in R.fwd_cap(128)] == [1024 * 128, 1024 * 128 + 1]
    assert [b * h * w for b, h, w in R.fwd_cap(256)] == [512 * 128, 512 * 128 + 1]
    assert {C for _, C in R.CASES_OUT} == {32, 64, 96, 128, 256}
    assert set(R.MSE_SHAPES) <= {s for s, C in R.CASES_OUT if C == 128}


# ----------------------------------------------------------------------------------------------------------------------
# (3) the conditions on the inputs, with the reference alone
# ----------------------------------------------------------------------------------------------------------------------
def _share(mask):
    return float(mask.double().mean())


def _dominated(frag, bound, want):
    """Share of outputs whose bound is more than half fragile terms, among outputs larger than their own fragile term."""
    return float(((frag > 0.5 * bound) & (want.abs() > frag)).double().mean())


@pytest.mark.parametrize("M,C", R.CASES_1X1, ids=lambda v: str(v))
def test_1x1_case_conditions(M, C):
    c = R.inputs_1x1(M, C)
    mean, invstd = R.host_stats(c.x)
    act = R.staged_activation(c.x, mean, invstd, c.gamma, c.beta)
    assert M == 1 or _share(act.fragile) <= SHARE, f"{c.tag}: fragile share of a = {_share(act.fragile):.2e}"
    m2, i2 = R.host_stats(c.h)
    _, dg2, db2, _ = BN.backward(c.h, c.dy, m2, i2, c.gamma2)
    dg2, db2 = dg2.float(), db2.float()
    for chain in (R.flat_chain(M, C), R.fused_chain(M)):
        assert chain < R.MAX_CHAIN, f"{c.tag}: an fp32 column-sum chain of {chain} additions"
    for chain in (R.wgrad_chain(M, C), R.fused_dw_chain(M)):
        assert R.sum_coef(chain) == (R.SUM_COEF if chain < R.MAX_CHAIN else chain * R.U32 * 1.1) >= chain * R.U32
    if M >= BIG:
        # counting on the staged operands is enough here: the element-wise parts of the backward, no GEMM
        sc = (c.gamma2 * i2).double()
        k1 = sc * i2.double() * dg2.double() / M
        dh = sc * (c.dy.double() - db2.double() / M) - k1 * (c.h.double() - m2.double())
        mag = sc.abs() * (c.dy.double().abs() + (db2.double() / M).abs()) + k1.abs() * (c.h.double().abs() + m2.double().abs())
        _, _, frag, _ = R.round_fragile(dh, mag)
        assert _share(frag) <= SHARE, f"{c.tag}: fragile share of dh = {_share(frag):.2e}"
        return
    fwd = R.conv1x1_forward(c.x, mean, invstd, c.gamma, c.beta, c.w, c.bias)
    assert M == 1 or _dominated(fwd.frag, R.mfma_bound(fwd.y, fwd.terms, fwd.frag, fwd.K, True), fwd.y) <= 0.01, f"{c.tag}: y"
    bwd = R.conv1x1_backward(c.h, c.dy, m2, i2, c.gamma2, dg2, db2, c.w)
    assert M == 1 or _share(bwd.fragile) <= SHARE, f"{c.tag}: fragile share of dh = {_share(bwd.fragile):.2e}"
    if M > 1:
        assert _dominated(bwd.dx_frag, R.mfma_bound(bwd.dx, bwd.dx_terms, bwd.dx_frag, bwd.K, True), bwd.dx) <= 0.01, f"{c.tag}: dx"
        dw, terms, frag = R.conv1x1_wgrad(bwd.dh_r, bwd.dh_delta, act)
        assert M < 4096 or _dominated(frag, R.sum_coef(R.fused_dw_chain(M)) * terms + frag, dw) <= 0.01, f"{c.tag}: dw"
        ps = R.prev_sums(c.x, R.rb(bwd.dx), mean, invstd, c.gamma, c.beta)
        assert float(((ps.flip_dbeta > R.SUM_COEF * ps.terms_dbeta) & (ps.dbeta.abs() > ps.flip_dbeta)).double().mean()) <= 0.05, f"{c.tag}: prev_dbeta"


@pytest.mark.parametrize("M,C", R.CASES_1X1, ids=lambda v: str(v))
def test_1x1_probe_is_exact_in_fp32(M, C):
    p = R.probe_1x1(M, C)
    for t in (p.x, p.dy):
        f = t.float()
        assert bool((f == f.round()).all()) and float(f.min()) >= 0 and float(f.max()) < 256, "not a small non-negative integer: inexact in bf16"
    x, dy = p.x.double(), p.dy.double()
    assert float(dy.sum(0).max()) < 2 ** 24 and float((dy * x).sum(0).max()) < 2 ** 24
    assert float(x.max() * dy.sum(0).max()) < 2 ** 24, "a dw entry's partial sums could leave the exact integers of fp32"
    assert bool((x[0] > 0).all()) and bool((x[M - 1] > 0).all()) and bool((dy[0] > 0).all()) and bool((dy[M - 1] > 0).all())


@pytest.mark.parametrize("shape,C", R.CASES_OUT, ids=lambda v: str(v).replace(" ", ""))
def test_output_case_conditions(shape, C):
    c = R.inputs_out(shape, C)
    mean, invstd = R.host_stats(c.u.reshape(-1, C))
    assert R.out_chain(*shape) < R.MAX_CHAIN and R.out_dw_chain(*shape) < R.MAX_CHAIN, f"{c.tag}: an fp32 chain past 300 additions"
    if c.M == 1:
        return          # exemption (a) of the module docstring
    if c.M >= BIG:
        act = R.staged_activation(c.u.reshape(-1, C), mean, invstd, c.gamma, c.beta)
        assert _share(act.fragile) <= SHARE, f"{c.tag}: fragile share of a = {_share(act.fragile):.2e}"
        return
    fwd = R.output_forward(c.u, mean, invstd, c.gamma, c.beta, c.w, c.bias)
    assert _share(fwd.act.fragile) <= SHARE, f"{c.tag}: fragile share of a = {_share(fwd.act.fragile):.2e}"
    assert _dominated(fwd.frag, R.mfma_bound(fwd.pre, fwd.terms, fwd.frag, fwd.K, False), fwd.pre) <= 0.01, f"{c.tag}: pre"
    o = R.output_backward(c.u, mean, invstd, c.gamma, c.beta, c.w, c.dy)
    assert _share(o.fragile) <= SHARE, f"{c.tag}: fragile ReLU decisions = {_share(o.fragile):.2e}"
    assert _dominated(o.du_flip, R.UB * o.du.abs() + o.du_own + o.du_flip, o.du) <= 0.01, f"{c.tag}: du"
    assert _dominated(o.dw_frag, R.SUM_COEF * o.dw_terms + o.dw_frag, o.dw) <= 0.01, f"{c.tag}: dw"


@pytest.mark.parametrize("shape,C", R.PROBE_OUT, ids=lambda v: str(v).replace(" ", ""))
def test_output_probe_is_exact_in_fp32(shape, C):
    p = R.probe_out(shape, C)
    for t in (p.u.float(), p.w, p.dy):
        assert bool((t == t.round()).all()) and float(t.abs().max()) < 256
    o = R.output_backward(p.u, p.zero, p.one, p.one, p.zero, p.w, p.dy, round_ops=True)
    fwd = R.output_forward(p.u, p.zero, p.one, p.one, p.zero, p.w, None)
    assert not bool(fwd.act.fragile.any()) and not bool(o.fragile.any()), "an integer operand next to a rounding decision"
    assert bool((fwd.pre == fwd.pre.round()).all()) and float(fwd.terms.max()) < 2 ** 24
    for sums in (o.dbeta_terms, o.dgamma_terms, o.dw_terms, o.dbias_terms):
        assert float(sums.max()) < 2 ** 24, "a partial sum could leave the exact integers of fp32"
    for v in (o.dbeta, o.dgamma, o.dw, o.dbias):
        assert bool((v == v.round()).all())
