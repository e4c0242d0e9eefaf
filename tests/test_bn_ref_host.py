"""The fp64 BatchNorm yardstick (tests/helpers/bn_ref64.py) checked on the CPU: against torch.autograd through F.batch_norm in
float64, at its M = 1 and zero-variance conventions, and -- on the very inputs the GPU envelope tests generate -- that the one
exclusion those tests permit (ReLU decisions within the fp32 rounding of the forward's expression) stays inside its cap."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import bn_ref64 as R


def _close(got, want, tol, what, scale=None):
    scale = max(float(want.abs().max()), 1e-300) if scale is None else scale
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("M,C", [(2, 4), (7, 8), (33, 12), (130, 24)])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_reference_matches_autograd_in_float64(M, C, relu, res):
    g = torch.Generator().manual_seed(100 * M + C)
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 1.3 + 0.4).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    r = torch.randn(M, C, generator=g, dtype=torch.float64)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64) + 0.5
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64) * 0.1, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm_t, rv_t, gamma, beta, True, R.MOMENTUM, R.EPS)
    pre = y
    if relu:
        y = F.relu(y)
    if res:
        y = y + F.relu(r)
    gx, gg, gb = torch.autograd.grad(y, [x, gamma, beta], dy)

    mean, invstd, (rm2, rv2) = R.stats(x, running=(rm, rv))
    _close(rm2, rm_t, 1e-12, "running_mean")
    _close(rv2, rv_t, 1e-12, "running_var")
    _close(mean, x.detach().mean(0), 1e-12, "mean")
    _close(invstd, 1.0 / torch.sqrt(x.detach().var(0, unbiased=False) + R.EPS), 1e-12, "invstd")
    got = R.apply(x, mean, invstd, gamma, beta, relu=relu, residual=r if res else None, relu_residual=res)
    _close(got, y.detach(), 1e-12, "forward")
    mask = R.relu_mask(x, mean, invstd, gamma, beta) if relu else None
    if relu:
        assert torch.equal(mask, pre.detach() > 0)
    dx, dgamma, dbeta, colsum = R.backward(x, dy, mean, invstd, gamma, mask)
    # dx's scale is that of its terms, gamma * invstd * dy: with two rows dy - mean(dy) - xhat * mean(dy * xhat) cancels to
    # almost nothing (xhat = +-1), and what is left of either evaluation is the rounding of the terms
    _close(dx, gx, 1e-12, "dx", scale=float((gamma.detach() * invstd).abs().max() * dy.abs().max()))
    _close(dgamma, gg, 1e-12, "dgamma")
    _close(dbeta, gb, 1e-12, "dbeta")
    _close(colsum, gx.sum(0), 1e-12, "dx_colsum", scale=float(M * (gamma.detach() * invstd).abs().max() * dy.abs().max()))
    # relu_out: max(0, .) of the final value
    got = R.apply(x, mean, invstd, gamma, beta, residual=r, relu_out=True)
    _close(got, F.relu(pre.detach() + r), 1e-12, "forward with relu_out")


def test_single_row_convention():
    """M = 1: the variance is 0, invstd = 1/sqrt(eps), running_var takes the biased variance (bn_stats_final_kernel: there is
    no unbiased one), and dx = 0 (dy - mean(dy) = 0 and xhat = 0)."""
    g = torch.Generator().manual_seed(1)
    x, dy = torch.randn(1, 8, generator=g), torch.randn(1, 8, generator=g)
    gamma, rm, rv = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g), torch.rand(8, generator=g) + 0.5
    mean, invstd, (rm2, rv2) = R.stats(x, running=(rm, rv))
    assert torch.equal(mean, x[0].double())
    assert torch.equal(invstd, torch.full((8,), 1.0 / R.EPS ** 0.5, dtype=torch.float64))
    assert torch.equal(rv2, (1.0 - R.MOMENTUM) * rv.double())
    assert torch.equal(rm2, (1.0 - R.MOMENTUM) * rm.double() + R.MOMENTUM * x[0].double())
    dx, dgamma, dbeta, colsum = R.backward(x, dy, mean, invstd, gamma)
    assert torch.equal(dx, torch.zeros(1, 8, dtype=torch.float64)) and torch.equal(colsum, torch.zeros(8, dtype=torch.float64))
    assert torch.equal(dbeta, dy[0].double()) and torch.equal(dgamma, torch.zeros(8, dtype=torch.float64))


def test_zero_variance_convention():
    """A constant column: mean is the constant, invstd = 1/sqrt(eps), xhat = 0, so dgamma = 0 and
    dx = gamma * invstd * (dy - mean(dy)); an all-zero column likewise."""
    d = R.special_inputs("constant")
    x, dy, gamma = d["x"], d["dy"], d["gamma"]
    mean, invstd, _ = R.stats(x)
    assert float(mean[0]) == 7.25 and float(mean[1]) == 0.0
    assert float(invstd[0]) == 1.0 / R.EPS ** 0.5 and float(invstd[1]) == 1.0 / R.EPS ** 0.5
    dx, dgamma, dbeta, _ = R.backward(x, dy, mean, invstd, gamma)
    assert float(dgamma[0]) == 0.0 and float(dgamma[1]) == 0.0
    want = gamma.double()[:2] * invstd[:2] * (dy.double()[:, :2] - dy.double()[:, :2].mean(0))
    _close(dx[:, :2], want, 1e-12, "dx of the constant columns")


def test_slab_walk_restated():
    assert R.slab_geom(1) == (1, 1) and R.slab_geom(64) == (1, 64) and R.slab_geom(65) == (2, 33)
    assert R.slab_geom(16453) == (258, 64) and R.slab_geom(40007) == (626, 64)
    assert R.slab_geom(65536) == (1024, 64) and R.slab_geom(70001) == (1015, 69) and R.slab_geom(87501) == (1018, 86)


@pytest.mark.parametrize("M,C,dt,data", R.case_ids(), ids=lambda v: str(v))
def test_fragile_relu_decisions_stay_inside_the_cap(M, C, dt, data):
    """The reference alone: on each GPU case's actual inputs, at most max(4, 1e-5 numel) elements have their ReLU decision
    within the fp32 rounding of the forward's expression.  (mean / invstd: the fp64 statistics rounded to fp32, which is what
    the kernels are handed up to the tolerance of bn_stats; the GPU test asserts the cap again with the values it uses.)"""
    assert R.chain_length(M, C, dt == R.BF16) < R.MAX_CHAIN
    d = R.make_inputs(M, C, dt, data)
    mean, invstd, _ = R.stats(d["x"])
    n = int(R.fragile(d["x"], R.round_f32(mean), R.round_f32(invstd), d["gamma"], d["beta"]).sum())
    assert n <= R.fragile_cap(M * C), f"{n} fragile elements of {M * C}"


def test_fragile_rule():
    """One column, hand-made: t = (x - 1) * 2 + beta.  With beta = 0 the sign of t is the sign of x - mean, which an fp32
    subtraction gets right: only t = 0 itself is fragile.  With beta != 0 it is the cancellation of the two magnitudes."""
    one = torch.ones(1, dtype=torch.float64)
    x = torch.tensor([[1.0], [1.0 + 4 * R.U32], [1.001], [0.0]], dtype=torch.float64)
    fr = R.fragile(x, one, 2 * one, one, 0 * one)
    assert fr[:, 0].tolist() == [True, False, False, False]
    # beta = -2 (x - mean) up to a relative 1e-7: cancellation to within the rounding of the two magnitudes
    fr = R.fragile(torch.tensor([[3.0]], dtype=torch.float64), one, 2 * one, one, -4 * one * (1 + 1e-7))
    assert bool(fr[0, 0])
    fr = R.fragile(torch.tensor([[3.0]], dtype=torch.float64), one, 2 * one, one, -4 * one * (1 + 1e-5))
    assert not bool(fr[0, 0])
