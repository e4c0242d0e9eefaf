"""The fp64 yardstick of the BatchNorm kernels (csrc/bn.hip) and the inputs of their envelope tests: plain torch on the CPU,
no F.batch_norm (ATen refuses M = 1 in training mode).  tests/test_bn_ref_host.py checks this file against torch.autograd;
tests/test_gpu_bn_envelope.py checks the kernels against it.  Tensors are [M][C]; every function widens what it is given to
float64, so a caller passes the operands as the kernel sees them (bf16 values rounded first)."""
import math

import torch

U32 = 2.0 ** -24                    # unit roundoff of fp32
EPS = 1e-5
MOMENTUM = 0.1
MAX_SLABS = 1024                    # bn.hip


def f64(t):
    return None if t is None else t.detach().to("cpu").double()


# ----------------------------------------------------------------------------------------------------------------------
# the operations
# ----------------------------------------------------------------------------------------------------------------------
def stats(x, eps=EPS, momentum=MOMENTUM, running=None):
    """-> mean, invstd, running' (None without running = (running_mean, running_var)).  The variance is two-pass about the mean;
    invstd uses the biased one, running_var the unbiased one -- and the biased one when M = 1, bn_stats_final_kernel's convention
    (a constant column or a single row gives invstd = 1 / sqrt(eps))."""
    x = f64(x)
    M = x.shape[0]
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    var_b = m2 / M
    invstd = 1.0 / torch.sqrt(var_b + eps)
    if running is None:
        return mean, invstd, None
    rm, rv = f64(running[0]), f64(running[1])
    var_u = m2 / (M - 1) if M > 1 else var_b
    return mean, invstd, ((1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * var_u)


def pre_activation(x, mean, invstd, gamma, beta):
    return (f64(x) - f64(mean)) * (f64(invstd) * f64(gamma)) + f64(beta)


def apply(x, mean, invstd, gamma, beta, relu=False, residual=None, relu_residual=False, relu_out=False):
    y = pre_activation(x, mean, invstd, gamma, beta)
    if relu:
        y = y.clamp_min(0.0)
    if residual is not None:
        r = f64(residual)
        y = y + (r.clamp_min(0.0) if relu_residual else r)
    if relu_out:
        y = y.clamp_min(0.0)
    return y


def relu_mask(x, mean, invstd, gamma, beta):
    """The mask of a fused BatchNorm + ReLU forward, decided in fp64."""
    return pre_activation(x, mean, invstd, gamma, beta) > 0.0


def backward(x, dy, mean, invstd, gamma, mask=None):
    """-> dx, dgamma, dbeta, dx_colsum of y = (x - mean) * invstd * gamma + beta with batch statistics; mask (bool [M][C] or
    None) is the ReLU that followed: dy counts where it is set."""
    x, g = f64(x), f64(dy)
    mean, invstd, gamma = f64(mean), f64(invstd), f64(gamma)
    M = x.shape[0]
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    xhat = (x - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * invstd * (g - dbeta / M - xhat * (dgamma / M))
    return dx, dgamma, dbeta, dx.sum(0)


def backward_terms(x, dy, mean, invstd, gamma, mask=None, dx=None):
    """sum |term| per column of the three sums of backward() (dgamma, dbeta, dx_colsum): the scale their fp32 bounds refer to;
    and, fourth, the column sums of |gamma invstd| (|dy| + |dbeta / M| + |xhat dgamma / M|), the magnitudes dx is formed from.
    dx: backward()'s, if the caller has it already."""
    x, g = f64(x), f64(dy)
    mean, invstd, gamma = f64(mean), f64(invstd), f64(gamma)
    M = x.shape[0]
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    xhat = (x - mean) * invstd
    if dx is None:
        dx = backward(x, dy, mean, invstd, gamma, mask)[0]
    parts = (gamma * invstd).abs() * (g.abs() + (g.sum(0) / M).abs() + (xhat * ((g * xhat).sum(0) / M)).abs())
    return (g * xhat).abs().sum(0), g.abs().sum(0), dx.abs().sum(0), parts.sum(0)


def fragile(x, mean, invstd, gamma, beta):
    """The one permitted exclusion.  The kernels decide the ReLU mask from t = (x - mean) * (invstd * gamma) + beta in fp32: a
    subtraction, the product invstd * gamma, a product and a sum, four roundings, each of at most 2^-24 of the magnitudes
    |x - mean| * invstd * |gamma| and |beta|.  Where fp64 puts |t| within twice that, either decision is correct."""
    x, mean, invstd, gamma, beta = f64(x), f64(mean), f64(invstd), f64(gamma), f64(beta)
    a = (x - mean).abs() * invstd * gamma.abs()
    t = (x - mean) * (invstd * gamma) + beta
    return t.abs() <= 8.0 * U32 * (a + beta.abs())


def fragile_cap(numel):
    return max(4, int(1e-5 * numel))


# ----------------------------------------------------------------------------------------------------------------------
# the slab walk of bn.hip (slab_geom), restated: where the ragged last slab begins, and how long the fp32 chains are
# ----------------------------------------------------------------------------------------------------------------------
def slab_geom(M):
    n = min(max(-(-M // 64), 1), MAX_SLABS)
    rows = -(-M // n)
    return -(-M // rows), rows          # nslab, rows per slab


def chain_length(M, C, bf16):
    """The longest chain of fp32 additions behind one column sum: a thread's share of a slab, then the row groups."""
    cw = C // (8 if bf16 else 4)
    rgroups = 256 // cw
    _, rows = slab_geom(M)
    return -(-rows // rgroups) + rgroups


# ----------------------------------------------------------------------------------------------------------------------
# the cases: (M, C, dtypes, what it reaches)
# ----------------------------------------------------------------------------------------------------------------------
F32, BF16 = "f32", "bf16"
BOTH = (F32, BF16)
CASES = [
    (1, 8, BOTH, "a single row: invstd = 1/sqrt(eps), dx = 0, running_var takes the biased variance"),
    (3, 8, BOTH, "fewer rows than row groups (fp32: 128 groups, bf16: 256)"),
    (5, 96, BOTH, "fewer rows than row groups at a non-power-of-two C (fp32: 10 groups, 16 idle threads)"),
    (64, 16, BOTH, "exactly one slab of 64 rows"),
    (65, 16, BOTH, "the 64/65 boundary: two slabs of 33 and 32 rows"),
    (130, 24, BOTH, "non-power-of-two C: fp32 CW = 6 (42 row groups, 4 idle threads), bf16 CW = 3 (85 groups, 1 idle)"),
    (130, 48, BOTH, "non-power-of-two C: fp32 CW = 12 (21 groups, 4 idle), bf16 CW = 6"),
    (130, 96, BOTH, "non-power-of-two C: fp32 CW = 24 (10 groups, 16 idle), bf16 CW = 12 (21 groups, 4 idle)"),
    (70, 1000, BOTH, "fp32 CW = 250: one row group, 6 idle threads; bf16 CW = 125: 2 groups, 6 idle (chain: 35 rows + 1)"),
    (70, 1020, (F32,), "fp32 CW = 255: one row group, one idle thread (1020 is no multiple of 8) (chain: 35 rows + 1)"),
    (70, 1024, BOTH, "the widest C: fp32 CW = 256 is one row group with no idle thread; bf16 two groups (chain: 35 rows + 1)"),
    (16453, 8, BOTH, "258 slabs of 64 rows, 5 in the last: the finalisers' second chunk holds two slabs (chain: 1 + 128 / 1 + 256)"),
    (40007, 24, BOTH, "626 slabs of 64 rows, 7 in the last: finaliser chunks 2 and 3 (chain fp32: 2 + 42, bf16: 1 + 85)"),
    (70001, 8, BOTH, "MAX_SLABS clamp: 69-row slabs, 1015 of them, 35 rows in the last; all 4 chunks (chain: 1 + 128 / 1 + 256)"),
    (70001, 4, (F32,), "the clamp at the narrowest fp32 C: CW = 1, 256 row groups (chain: 1 + 256)"),
    (44001, 96, (F32,), "bn_apply grid stride in fp32: M C / 4 = 1 056 024 > 4096 * 256, mult = 3 -> 4098 blocks (chain: 7 + 10)"),
    (87501, 96, (BF16,), "bn_apply grid stride in bf16: M C / 8 = 1 050 012 > 4096 * 256, mult = 3 -> 4098 blocks (chain: 5 + 21)"),
]
MIXED_CASES = [(130, 96), (1000, 128)]          # bn_apply fp32 -> bf16 and bf16 -> fp32, both with a residual
SPECIAL_MC = (5000, 8)                          # the two special-column cases (chain: 1 + 128)
MAX_CHAIN = 300                                 # 300 * 2^-24 = 1.8e-5 < the 2e-5 of the fp32 sums' bound


def case_ids():
    return [(M, C, dt, data) for M, C, dts, _ in CASES for dt in dts for data in ("gauss", "int")]


def torch_dtype(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def _seed(M, C, dt, data):
    return 1000003 * M + 1009 * C + (17 if dt == BF16 else 0) + (5 if data == "int" else 0)


def make_inputs(M, C, dt, data):
    """The inputs of one case, in their storage type, as the GPU tests upload them (one generator, fixed draw order).
    gauss: x = 1.3 randn + 0.4, dy = randn + 0.5 (non-zero means: the sums are not cancellation noise).
    int:   x in {-3..3}, dy in {-2..2}, integer-valued: every fp32 partial sum of dy is exact.  dy is non-zero and x is +-3 on
           the first and last row of the tensor and of the last slab, so a dropped or doubled row there changes dbeta and mean."""
    g = torch.Generator().manual_seed(_seed(M, C, dt, data))
    td = torch_dtype(dt)
    if data == "gauss":
        x = torch.randn(M, C, generator=g) * 1.3 + 0.4
        dy = torch.randn(M, C, generator=g) + 0.5
        res = torch.randn(M, C, generator=g)
    else:
        x = torch.randint(-3, 4, (M, C), generator=g).float()
        dy = torch.randint(-2, 3, (M, C), generator=g).float()
        res = torch.randint(-3, 4, (M, C), generator=g).float()
        nslab, rows = slab_geom(M)
        for k, r in enumerate(sorted({0, M - 1, (nslab - 1) * rows})):
            dy[r] = torch.tensor([1.0, -2.0, 2.0, 1.0]).repeat(C // 4) * (1 if k % 2 == 0 else -1)
            x[r] = torch.tensor([3.0, -3.0, 3.0, 3.0]).repeat(C // 4)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm = torch.randn(C, generator=g) * 0.1
    rv = torch.rand(C, generator=g) + 0.5
    return dict(x=x.to(td), dy=dy.to(td), res=res.to(td), gamma=gamma, beta=beta, rm=rm, rv=rv)


def special_inputs(kind):
    """(5000, 8) fp32.  'offset': x = 0.5 randn + 1000, a mean that dwarfs the spread (E[x^2] - E[x]^2 in fp32 has lost the
    variance: 1e6 * 2^-24 = 0.06 against 0.25).  'constant': column 0 is 7.25 throughout, column 1 is zero throughout."""
    M, C = SPECIAL_MC
    g = torch.Generator().manual_seed(77 if kind == "offset" else 78)
    if kind == "offset":
        x = torch.randn(M, C, generator=g) * 0.5 + 1000.0
    else:
        x = torch.randn(M, C, generator=g) * 1.3 + 0.4
        x[:, 0] = 7.25
        x[:, 1] = 0.0
    dy = torch.randn(M, C, generator=g) + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    return dict(x=x, dy=dy, gamma=gamma, beta=beta)


def round_f32(t):
    """fp64 -> the nearest fp32, as a stand-in on the CPU for the fp32 mean / invstd the kernels are handed."""
    return t.float()


assert math.isclose(U32, 5.9604644775390625e-08)
