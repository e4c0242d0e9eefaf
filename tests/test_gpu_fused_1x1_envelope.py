"""The ResBlock's 1x1 convolution with BatchNorm arithmetic in its operand staging (csrc/gemm_flat.hip; the BatchNorm-on-load Q
operand of csrc/gemm_wgrad.hip) over its envelope, against the fp64 yardstick tests/helpers/fused_ref64.py.

C: 32, 64, 128, 256 -- all of nsg_bn_relu_conv1x1_supported.  C = 256 runs flat_wide_kernel (64-row tiles, 8 waves, at most 256
blocks), the others flat_gemm_kernel (128-row tiles, at most 512 persistent blocks).  M on each side of every boundary:
    1, 31                       below one wave's 32 rows
    127 | 128 | 129             one tile | two (C = 256: 63 | 64 | 65)
    256 | 257                   nsg_bn_relu_conv1x1_wgrad's first slab split (slabs of at least 256 rows)
    65536 | 65537               a persistent block takes a second tile (C = 256: 16384 | 16385)
    32768 | 32769               the same for nsg_bn_backward_conv1x1_dgrad_wgrad (C = 128, 256 blocks)
    130817 (C = 256: 32513)     the weight gradient reaches its slab cap (512 slabs; 128 at C = 256)
    196685                      three to four tiles per block, the last tile ragged (C = 128)
every M at C = 128, the boundary set at C = 256 and C = 32, and 1, 129, 65537 at C = 64 (fused_ref64.CASES_1X1;
tests/test_fused_ref_host.py derives the table from the kernels' constants and checks the inputs' conditions on the CPU).

Inputs: x, h ~ N(0.4, 1.3^2) as bf16, per-channel gamma ~ U(0.5, 1.5), beta ~ N(0, 0.3^2); channel 1 has beta = -8 (the ReLU passes
almost nothing), channel 2 is 6 +- 0.2 (mean >> std); w ~ N(0, 0.15^2), dy ~ N(0, 1).  Statistics come from ops.bn_stats and
dgamma / dbeta from ops.bn_backward_sums: the fp32 values the kernels are handed, which the reference widens.

Bounds against fp64 (the classes of tests/test_gpu_bn_envelope.py; derived in fused_ref64.py, none tuned against the kernels):
  y, dx           MFMA outputs stored bf16: 2^-8 |want| + (C + 4) 2^-24 sum |term| + the fragile operands' part.  The reference
                  multiplies the SAME bf16-rounded operands (a, dh, w) the kernels do.
  dh              the staged operand as stored: 2^-8 |want| + 8 * 2^-24 of the magnitudes it is formed from
  fp32 sums       dh_colsum, prev_dgamma / prev_dbeta, dw: 2e-5 sum |term| for chains below 300 additions (the chain's own
                  coefficient, chain * 2^-24 * 1.1, where it is longer: the weight gradients, whose accumulators run over a slab's
                  or a block's rows and whose partials are added in fp32) + own + the fragile ReLU decisions' whole terms.
                  dh_colsum sums dh BEFORE its store rounding: own = 8 * 2^-24 of dh's magnitudes.  prev_* sum dx AS STORED:
                  the reference sums the stored dx (checked by itself against fp64 just before), so own = 0 -- summing the
                  unrounded fp64 dx instead would put M store roundings of 2^-8 |dx| into a bound of 2e-5 M |dx|.
                  nsg_bn_relu_conv1x1_wgrad is handed the REFERENCE's bf16 dh, so only a is fragile there; the one-pass form
                  forms dh itself: both operands.
  statistics      of y as stored (fp64 over the kernel's own y): mean rtol 1e-5 + atol (2e-6 std + 1e-6), invstd rtol 2e-5,
                  running statistics rtol 1e-5 + atol 1e-6
  integer probe   identity BatchNorm, w = I, x and dy in {0..3}: y = x, dh = dx = dy bit for bit; dh_colsum, prev_dbeta,
                  prev_dgamma and every dw entry EQUAL the integer sums; mean_y within 4 * 2^-24 max |y|.  A lost or doubled row
                  of 65 537 is invisible to 2e-5 and far outside these.
Every output is allocated over NaN poison, every [M][C] output is a view of a buffer with one tile of canary rows behind row M
which must be unchanged, two runs give the same bits, the prev_* form gives the dh / dx bits of the plain form, the one-pass form
the dx bits of the two-kernel form.

Largest error / bound per class as measured on an MI355X (also DESIGN.md, "Envelope of the fused BatchNorm + conv operators"):
y / dx 0.995 (M=65537 C=32 y) and dh 0.996 (M=196685 C=128), both the bf16 store rounding itself; dw 0.885 (M=129 C=128, one
pass: a fragile operand's term); fp32 sums 0.062 (M=1 C=128 dh_colsum); statistics 0.025 (M=32513 C=256 running_mean).  The integer
probes are exact at every M."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, ops  # noqa: E402
from tests.helpers import bn_ref64 as BN  # noqa: E402
from tests.helpers import fused_ref64 as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
BF = torch.bfloat16
WORST = {}


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _within(cls, got, want, bound, what):
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (an element the kernel did not write?)"
    err = (got.reshape(want.shape) - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[fused 1x1] {what}: error / bound = {ratio:.4f}")
    _note(cls, ratio, what)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def _rows(C):
    return R.WIDE_ROWS if C == 256 else R.FLAT_ROWS


def _tensor(M, C):
    """A bf16 [M][C] output over NaN poison with one tile of canary rows behind it -> (the view, the whole buffer)."""
    whole = torch.full((M + _rows(C), C), NAN, dtype=BF, device=DEV)
    return whole[:M], whole


def _canaries_intact(whole, M, what):
    tail = whole[M:].view(torch.int16)
    assert bool((tail == tail.new_full((), 0x7FC0)).all()), f"{what}: rows past M were written"


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _ws(query, M, C):
    return ops._ws(torch.device(DEV), query, M, C)


# ---- the entry points on caller-owned outputs (ops.* allocates its own) -----------------------------------------------------------
def forward(x, mean, invstd, gamma, beta, w, bias, stats=None):
    M, C = x.shape
    y, whole = _tensor(M, C)
    ws, nb = _ws("nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    p = ops._p
    if stats is None:
        _lib.call("nsg_bn_relu_conv1x1_forward", p(x), p(mean), p(invstd), p(gamma), p(beta), p(w), p(bias), p(y), M, C, ops.NSG_BF16, p(ws), nb,
                  ops._stream())
        out = (y,)
    else:
        my, iy = _nan(C), _nan(C)
        _lib.call("nsg_bn_relu_conv1x1_forward_bnstats", p(x), p(mean), p(invstd), p(gamma), p(beta), p(w), p(bias), p(y), BN.EPS, BN.MOMENTUM,
                  p(my), p(iy), p(stats[0]), p(stats[1]), M, C, ops.NSG_BF16, p(ws), nb, ops._stream())
        out = (y, my, iy)
    torch.cuda.synchronize()
    _canaries_intact(whole, M, "y")
    return out


def dgrad(h, dy, mean, invstd, gamma, dgamma, dbeta, w, prev=None):
    M, C = h.shape
    (dh, dh_all), (dx, dx_all) = _tensor(M, C), _tensor(M, C)
    cs = _nan(C)
    pdg, pdb = (_nan(C), _nan(C)) if prev is not None else (None, None)
    px, pm, pi, pg, pb = prev if prev is not None else (None,) * 5
    ws, nb = _ws("nsg_bn_relu_conv1x1_workspace_bytes", M, C)
    p = ops._p
    _lib.call("nsg_bn_backward_conv1x1_dgrad", p(h), p(dy), p(mean), p(invstd), p(gamma), p(dgamma), p(dbeta), p(w), p(dh), p(dx), p(cs), p(px),
              p(pm), p(pi), p(pg), p(pb), p(pdg), p(pdb), M, C, ops.NSG_BF16, p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    _canaries_intact(dh_all, M, "dh")
    _canaries_intact(dx_all, M, "dx")
    return dh, dx, cs, pdg, pdb


def dgrad_wgrad(h, dy, mean, invstd, gamma, dgamma, dbeta, w, prev):
    M, C = h.shape
    dx, dx_all = _tensor(M, C)
    dw, cs, pdg, pdb = _nan(C, C, 1, 1), _nan(C), _nan(C), _nan(C)
    px, pm, pi, pg, pb = prev
    ws, nb = _ws("nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes", M, C)
    p = ops._p
    _lib.call("nsg_bn_backward_conv1x1_dgrad_wgrad", p(h), p(dy), p(mean), p(invstd), p(gamma), p(dgamma), p(dbeta), p(w), p(dx), p(dw), p(cs),
              p(px), p(pm), p(pi), p(pg), p(pb), p(pdg), p(pdb), M, C, ops.NSG_BF16, p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    _canaries_intact(dx_all, M, "dx (one pass)")
    return dx, dw, cs, pdg, pdb


def wgrad(x, mean, invstd, gamma, beta, dy):
    C = x.shape[1]
    return ops.bn_relu_conv1x1_wgrad(x, mean, invstd, gamma, beta, dy, dw=_nan(C, C, 1, 1))


def _same(a, b, what):
    for u, v in zip(a, b):
        if u is not None:
            assert torch.equal(u.view(torch.int16) if u.dtype == BF else u, v.view(torch.int16) if v.dtype == BF else v), what


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=R.CASES_1X1, ids=lambda p: f"M{p[0]}-C{p[1]}")
def case(request):
    M, C = request.param
    c = R.inputs_1x1(M, C)
    c.g = types.SimpleNamespace(**{n: getattr(c, n).to(DEV) for n in ("x", "h", "dy", "w", "bias", "gamma", "beta", "gamma2", "rm", "rv")})
    g = c.g
    g.mean, g.invstd = ops.bn_stats(g.x, C)
    g.m2, g.i2 = ops.bn_stats(g.h, C)
    g.dg2, g.db2 = ops.bn_backward_sums(g.h, g.dy, g.m2, g.i2, g.gamma2)
    c.front = (g.x, g.mean, g.invstd, g.gamma, g.beta)
    c.act = R.staged_activation(c.x, g.mean, g.invstd, c.gamma, c.beta)
    return c


def test_forward(case):
    c, g = case, case.g
    args = (g.x, g.mean, g.invstd, g.gamma, g.beta, g.w, g.bias)
    (y,) = forward(*args)
    _same((y,), forward(*args), "two runs of the forward differ")
    rm, rv = g.rm.clone(), g.rv.clone()
    y_s, my, iy = forward(*args, stats=(rm, rv))
    _same((y_s,), (y,), "the _bnstats form stores another y")
    ref = R.conv1x1_forward(c.x, g.mean, g.invstd, c.gamma, c.beta, c.w, c.bias)
    _within("y, dx", y, ref.y, R.mfma_bound(ref.y, ref.terms, ref.frag, ref.K, True), c.tag + " y")
    # the store-phase statistics describe y AS STORED
    mean64, invstd64, (rm64, rv64) = BN.stats(y.cpu(), running=(c.rm, c.rv))
    std = torch.sqrt((1.0 / invstd64 ** 2 - BN.EPS).clamp_min(0.0))
    _within("statistics", my, mean64, 1e-5 * mean64.abs() + 2e-6 * std + 1e-6, c.tag + " mean_y")
    _within("statistics", iy, invstd64, 2e-5 * invstd64, c.tag + " invstd_y")
    _within("statistics", rm, rm64, 1e-5 * rm64.abs() + 1e-6, c.tag + " running_mean")
    _within("statistics", rv, rv64, 1e-5 * rv64.abs() + 1e-6, c.tag + " running_var")


def test_backward(case):
    c, g = case, case.g
    M, C = c.M, c.C
    args = (g.h, g.dy, g.m2, g.i2, g.gamma2, g.dg2, g.db2, g.w)
    dh, dx, cs, _, _ = dgrad(*args)
    _same((dh, dx, cs), dgrad(*args)[:3], "two runs of the data gradient differ")
    dh_b, dx_b, cs_b, pdg, pdb = dgrad(*args, prev=c.front)
    _same((dh_b, dx_b, cs_b), (dh, dx, cs), "the prev_* form gives other dh / dx bits than the plain form")
    ref = R.conv1x1_backward(c.h, c.dy, g.m2, g.i2, c.gamma2, g.dg2, g.db2, c.w)
    _within("dh", dh, ref.dh, R.UB * ref.dh.abs() + R.WINDOW * ref.dh_mag, c.tag + " dh")
    _within("y, dx", dx, ref.dx, R.mfma_bound(ref.dx, ref.dx_terms, ref.dx_frag, ref.K, True), c.tag + " dx")
    coef = R.sum_coef(R.flat_chain(M, C))
    _within("fp32 sums", cs, ref.colsum, coef * ref.colsum_terms + ref.colsum_own, c.tag + " dh_colsum")
    ps = R.prev_sums(c.x, dx.cpu(), g.mean, g.invstd, c.gamma, c.beta)
    b_dg, b_db = coef * ps.terms_dgamma + ps.flip_dgamma, coef * ps.terms_dbeta + ps.flip_dbeta
    _within("fp32 sums", pdg, ps.dgamma, b_dg, c.tag + " prev_dgamma")
    _within("fp32 sums", pdb, ps.dbeta, b_db, c.tag + " prev_dbeta")
    # nsg_bn_backward_sums on (prev_x, the stored dx) is in the same class
    sdg, sdb = ops.bn_backward_sums(g.x, dx.contiguous(), g.mean, g.invstd, g.gamma, relu_beta=g.beta)
    _within("fp32 sums", sdg, ps.dgamma, b_dg, c.tag + " bn_backward_sums dgamma on the stored dx")
    _within("fp32 sums", sdb, ps.dbeta, b_db, c.tag + " bn_backward_sums dbeta on the stored dx")
    # the weight gradient on the reference's bf16 dh: only a is fragile
    dw = wgrad(*c.front, ref.dh_r.to(BF).to(DEV))
    dw64, terms, frag = R.conv1x1_wgrad(ref.dh_r, None, c.act)
    _within("dw", dw, dw64, R.sum_coef(R.wgrad_chain(M, C)) * terms + frag, c.tag + " dw (nsg_bn_relu_conv1x1_wgrad)")
    assert ops.bn_backward_conv1x1_dgrad_wgrad_supported(BF, C) == (C == 128)
    if C != 128:
        return
    one = dgrad_wgrad(*args, c.front)
    _same(one, dgrad_wgrad(*args, c.front), "two runs of the one-pass form differ")
    dx_f, dw_f, cs_f, pdg_f, pdb_f = one
    _same((dx_f,), (dx,), "the one-pass form gives other dx bits than the two-kernel form")
    coef = R.sum_coef(R.fused_chain(M))
    _within("fp32 sums", cs_f, ref.colsum, coef * ref.colsum_terms + ref.colsum_own, c.tag + " dh_colsum (one pass)")
    _within("fp32 sums", pdg_f, ps.dgamma, coef * ps.terms_dgamma + ps.flip_dgamma, c.tag + " prev_dgamma (one pass)")
    _within("fp32 sums", pdb_f, ps.dbeta, coef * ps.terms_dbeta + ps.flip_dbeta, c.tag + " prev_dbeta (one pass)")
    dw64, terms, frag = R.conv1x1_wgrad(ref.dh_r, ref.dh_delta, c.act)
    _within("dw", dw_f, dw64, R.sum_coef(R.fused_dw_chain(M)) * terms + frag, c.tag + " dw (one pass)")


@pytest.mark.parametrize("M,C", R.CASES_1X1, ids=lambda v: str(v))
def test_integer_probe(M, C):
    """Identity BatchNorm and w = I: every output is an integer the kernels must reproduce exactly."""
    p = R.probe_1x1(M, C)
    x, dy, w, zero, one = (t.to(DEV) for t in (p.x, p.dy, p.w, p.zero, p.one))
    x64, dy64 = p.x.double(), p.dy.double()
    y, my, iy = forward(x, zero, one, one, zero, w, None, stats=(None, None))
    assert torch.equal(y, x), f"{p.tag}: y != x"
    assert float((my.double().cpu() - x64.mean(0)).abs().max()) <= 4 * R.U32 * float(x64.max()), f"{p.tag}: mean_y"
    front = (x, zero, one, one, zero)
    dh, dx, cs, pdg, pdb = dgrad(x, dy, zero, one, one, zero, zero, w, prev=front)
    assert torch.equal(dh, dy) and torch.equal(dx, dy), f"{p.tag}: dh / dx != dy"
    g64 = dy64 * (x64 > 0)
    exact = lambda got, want, what: torch.testing.assert_close(got.double().cpu().reshape(want.shape), want, rtol=0, atol=0,  # noqa: E731
                                                               msg=lambda m: f"{p.tag} {what}: {m}")
    exact(cs, dy64.sum(0), "dh_colsum")
    exact(pdb, g64.sum(0), "prev_dbeta")
    exact(pdg, (g64 * x64).sum(0), "prev_dgamma")
    dw64 = dy64.t() @ x64
    exact(wgrad(*front, dy), dw64, "dw (nsg_bn_relu_conv1x1_wgrad)")
    if C == 128:
        dx_f, dw_f, cs_f, pdg_f, pdb_f = dgrad_wgrad(x, dy, zero, one, one, zero, zero, w, front)
        assert torch.equal(dx_f, dy), f"{p.tag}: dx (one pass) != dy"
        exact(dw_f, dw64, "dw (one pass)")
        exact(cs_f, dy64.sum(0), "dh_colsum (one pass)")
        exact(pdb_f, g64.sum(0), "prev_dbeta (one pass)")
        exact(pdg_f, (g64 * x64).sum(0), "prev_dgamma (one pass)")


def test_rejections_launch_nothing():
    """Every refusal raises NsgError before anything is launched: the outputs keep their poison."""
    def refused(fn, *outs):
        with pytest.raises(_lib.NsgError):
            fn()
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o.float()).all()), "a refused call wrote to its output"

    def call_forward(x, C, y, ws_short=0, dtype=BF, w=None, M=None):
        M = x.shape[0] if M is None else M
        v = torch.ones(C, device=DEV)
        w = torch.zeros(C, C, 1, 1, device=DEV) if w is None else w
        ws, nb = _ws("nsg_bn_relu_conv1x1_workspace_bytes", max(M, 1), C if ops.bn_relu_conv1x1_supported(BF, C) else 128)
        p = ops._p
        _lib.call("nsg_bn_relu_conv1x1_forward", p(x), p(v), p(v), p(v), p(v), p(w), p(None), p(y), M, C, ops.nsg_dtype(dtype), p(ws), nb - ws_short,
                  ops._stream())

    M = 40
    for C in (96, 512):
        assert not ops.bn_relu_conv1x1_supported(BF, C)
        x, y = torch.ones(M, C, dtype=BF, device=DEV), torch.full((M, C), NAN, dtype=BF, device=DEV)
        refused(lambda: call_forward(x, C, y), y)
    C = 64
    x, y = torch.ones(M, C, dtype=BF, device=DEV), torch.full((M, C), NAN, dtype=BF, device=DEV)
    assert not ops.bn_relu_conv1x1_supported(torch.float32, C)
    refused(lambda: call_forward(x.float(), C, y, dtype=torch.float32), y)
    refused(lambda: call_forward(x, C, y, M=0), y)
    refused(lambda: call_forward(x, C, y, ws_short=1), y)
    flat = torch.ones(M * C + 8, dtype=BF, device=DEV)
    yflat = torch.full((M * C + 8,), NAN, dtype=BF, device=DEV)
    refused(lambda: call_forward(flat[1:M * C + 1].view(M, C), C, y), y)                    # x off 16-byte alignment
    refused(lambda: call_forward(x, C, yflat[1:M * C + 1].view(M, C)), yflat)               # y off it
    # the data gradient and the weight gradient: misaligned operands, short workspace
    v, z = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    w = torch.zeros(C, C, 1, 1, device=DEV)
    mis = flat[1:M * C + 1].view(M, C)
    with pytest.raises(_lib.NsgError):
        ops.bn_backward_conv1x1_dgrad(mis, x, z, v, v, z, z, w)
    with pytest.raises(_lib.NsgError):
        ops.bn_backward_conv1x1_dgrad(x, mis, z, v, v, z, z, w)
    with pytest.raises(_lib.NsgError):
        ops.bn_backward_conv1x1_dgrad(x, x, z, v, v, z, z, w, prev=(mis, z, v, v, z))
    dw = _nan(C, C, 1, 1)
    refused(lambda: ops.bn_relu_conv1x1_wgrad(mis, z, v, v, z, x, dw=dw), dw)
    refused(lambda: ops.bn_relu_conv1x1_wgrad(x, z, v, v, z, mis, dw=dw), dw)
    # the one-pass form: C = 128 only, the BatchNorm in front required
    assert not ops.bn_backward_conv1x1_dgrad_wgrad_supported(BF, 64)
    with pytest.raises(_lib.NsgError):
        ops.bn_backward_conv1x1_dgrad_wgrad(x, x, z, v, v, z, z, w, (x, z, v, v, z))
    C = 128
    x = torch.ones(M, C, dtype=BF, device=DEV)
    v, z, w = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, C, 1, 1, device=DEV)
    dx, dw = torch.full((M, C), NAN, dtype=BF, device=DEV), _nan(C, C, 1, 1)
    ws, nb = _ws("nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes", M, C)
    p = ops._p

    def one_pass(px, nbytes):
        _lib.call("nsg_bn_backward_conv1x1_dgrad_wgrad", p(x), p(x), p(z), p(v), p(v), p(z), p(z), p(w), p(dx), p(dw), p(None), p(px), p(z), p(v), p(v),
                  p(z), p(z.clone()), p(z.clone()), M, C, ops.NSG_BF16, p(ws), nbytes, ops._stream())

    refused(lambda: one_pass(None, nb), dx, dw)
    refused(lambda: one_pass(x, nb - 1), dx, dw)


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[fused 1x1 summary] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
