"""The streaming kernels of csrc/elementwise.hip over their envelope: every storage type, the scalar and the 16-byte path of each
launcher, the scalar fallback for a misaligned pointer, and lengths beyond one grid (4096 blocks of 256 threads, or the 1024
blocks of the loss reductions), where a thread takes a second element.

Bounds (none is tuned against the kernels):
  exact                    relu_backward_add, convert, add, add_per_clip, codebook_grad_from_sums, increment_counters: the bits of
                           the same fp32 operations on the CPU, rounded once to the storage type
  tanh_backward            the existing rtol 1e-6 + atol 1e-7 against fp64 (why |g| <= 3: see the test)
  fp32 sums (clip_colsum)  2e-5 * sum |term|: a thread's share of a clip slab + the row groups + 16 slabs stay below 300 chained
                           additions (300 * 2^-24 = 1.8e-5); the integer probe demands equality
  losses                   rtol 1e-6 (the existing figure; derived: d and d*d round once each in fp32, the sum is double, the mean
                           rounds once: 3 * 2^-24 = 1.8e-7); with integer operands the loss equals np.float32(S / n) exactly
  loss gradients           4 * 2^-24 of the magnitudes of the terms + the rounding of d = a - c itself (2^-24 max(|a|, |c|) times
                           the scale); stored bf16: 2^-8 |want| more
  adam                     m, v within 4 * 2^-24 relative + the smallest normal; |p - p64| <= 2^-24 |p64| + 8 * 2^-24 |update64|"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402

DEV = "cuda:0"
U32 = 2.0 ** -24
BF16_HALF_ULP = 2.0 ** -8
TINY32 = float(np.finfo(np.float32).tiny)
GRID = 4096 * 256          # threads of a full grid: beyond it the grid-stride loops run a second time
RED = 1024 * 256           # ... and of the loss reductions (RED_BLOCKS)
F32, BF16 = torch.float32, torch.bfloat16
DT = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
WORST = {}


def gpu(t):
    return t.to(DEV).contiguous()


def width(*dts):
    return 8 if BF16 in dts else 4


def lengths(W):
    """1, 3, 1001: scalar path; 4096: 16-byte path; GRID + 77: scalar path with a grid stride; W (GRID + 300): 16-byte path
    with a grid stride."""
    return [1, 3, 1001, 4096, GRID + 77, W * (GRID + 300)]


def mis(t):
    """t's values in a contiguous view that starts at element 1 of a larger buffer: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def nan_like(t, dtype=None):
    return torch.full(t.shape, float("nan"), dtype=dtype or t.dtype, device=DEV)


def poison(shape, dtype):
    """The next torch.empty of this size is most likely handed this block: an element the kernel leaves unwritten reads NaN."""
    t = torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV)
    del t


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    a, b = bits(got), bits(want)
    if not torch.equal(a, b):
        bad = (a != b).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} elements differ, first at {i}: got "
                             f"{float(got.flatten()[i].float())!r}, want {float(want.flatten()[i].float())!r}")


def note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def within(cls, got, want, bound, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got.detach().double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    note(cls, ratio, what)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def twice(fn):
    a, b = fn(), fn()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (u is None and v is None) or torch.equal(u, v), "two runs of the same call differ"
    return a


# ----------------------------------------------------------------------------------------------------------------------
# relu_backward_add
# ----------------------------------------------------------------------------------------------------------------------
def _relu_bwd_ref(a, b, x):
    s = a.float() + b.float() if b is not None else a.float()          # fp32 on both sides; one rounding to the storage type
    return torch.where(x.float() > 0, s, torch.zeros_like(s)).to(a.dtype)


def _relu_bwd_inputs(n, dt):
    g = torch.Generator().manual_seed(n + (1 if dt == BF16 else 0))
    a, b, x = (torch.randn(n, generator=g).to(dt) for _ in range(3))
    x[0] = 0.0              # x = 0 and x = -0 pass nothing
    x[-1] = -0.0
    return a, b, x


@DT
@pytest.mark.parametrize("n_of_w", range(6), ids=["1", "3", "1001", "4096", "grid+77", "w*(grid+300)"])
def test_relu_backward_add(n_of_w, dt):
    n = lengths(width(dt))[n_of_w]
    a, b, x = _relu_bwd_inputs(n, dt)
    ag, bg, xg = gpu(a), gpu(b), gpu(x)
    for bb, bbg in ((b, bg), (None, None)):
        got = twice(lambda: ops.relu_backward_add(ag, bbg, xg, out=nan_like(xg)))
        assert_bits(got, _relu_bwd_ref(a, bb, x), f"relu_backward_add n={n} b={'given' if bb is not None else None}")


@DT
def test_relu_backward_add_misaligned(dt):
    """Any one misaligned pointer sends the call down the scalar kernel: the bits of the aligned call."""
    n = 4096
    a, b, x = _relu_bwd_inputs(n, dt)
    ag, bg, xg = gpu(a), gpu(b), gpu(x)
    want = ops.relu_backward_add(ag, bg, xg)
    assert_bits(want, _relu_bwd_ref(a, b, x), "aligned")
    for k in range(4):
        args = [ag, bg, xg]
        out = nan_like(xg)
        if k < 3:
            args[k] = mis(args[k])
        else:
            out = mis(out)
        assert_bits(ops.relu_backward_add(*args, out=out), want.cpu(), f"relu_backward_add with misaligned pointer {k}")
    assert_bits(ops.relu_backward_add(mis(ag), None, mis(xg), out=mis(nan_like(xg))), _relu_bwd_ref(a, None, x), "all misaligned, b=None")


# ----------------------------------------------------------------------------------------------------------------------
# convert
# ----------------------------------------------------------------------------------------------------------------------
def _convert_values(n, src, seed):
    """fp32 values on which a bf16 rounding goes wrong if it can: round-to-even ties both ways (1 + 2^-8 -> 1, 1 + 3 2^-8 ->
    1 + 2^-6), their neighbours one fp32 ulp below and above, +-0, +-inf, the largest finite fp32 (-> inf), the largest bf16
    and the tie above it, a carry into the exponent, the smallest normal; then ties at random exponents (low half = 0x8000)
    and random values over 60 decades.  No NaN and no fp32 denormal."""
    g = torch.Generator().manual_seed(seed)
    f = np.float32
    base = [f(1 + 2.0 ** -8), f(1 + 3 * 2.0 ** -8), np.nextafter(f(1 + 2.0 ** -8), f(0)), np.nextafter(f(1 + 2.0 ** -8), f(2)),
            np.nextafter(f(1 + 3 * 2.0 ** -8), f(0)), np.nextafter(f(1 + 3 * 2.0 ** -8), f(2)), f(0.0), f(-0.0), f(np.inf), f(-np.inf),
            np.finfo(f).max, -np.finfo(f).max, f(3.3895313892515355e38), f(3.3961775292304601e38), np.nextafter(f(2), f(0)),
            np.finfo(f).tiny, -np.finfo(f).tiny, f(1 + 2.0 ** -7), f(0.5 + 2.0 ** -9), f(0.5 + 3 * 2.0 ** -9)]
    sp = torch.tensor(np.array(base + [-v for v in base[:6]], dtype=np.float32))
    k = min(n, 512)
    rb = torch.randn(k, generator=g).bfloat16().float() * (10.0 ** torch.randint(-30, 31, (k,), generator=g).float())
    rb = rb.bfloat16().float()
    ties = (rb.view(torch.int32) | 0x8000).view(torch.float32)          # exactly half way between two bf16 values
    rnd = torch.randn(n, generator=g) * (10.0 ** torch.randint(-30, 31, (n,), generator=g).float())
    v = torch.cat([sp, ties, rnd])[:n].clone()
    v = torch.where((v != 0) & (v.abs() < TINY32), torch.ones_like(v), v)
    assert not bool(torch.isnan(v).any())
    return v if src == F32 else v.bfloat16()


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)], ids=["f32_bf16", "bf16_f32", "f32_f32", "bf16_bf16"])
@pytest.mark.parametrize("n_of_w", range(6), ids=["1", "3", "1001", "4096", "grid+77", "w*(grid+300)"])
def test_convert(n_of_w, src, dst):
    n = lengths(width(src, dst))[n_of_w]
    v = _convert_values(n, src, seed=n)
    vg = gpu(v)
    for relu in (False, True):
        w = torch.where(v.float() > 0, v.float(), torch.zeros(1)) if relu else v.float()          # max(v, 0): +0 for -0 and below
        want = w.to(dst)                                                                          # torch's CPU cast: round to nearest even
        got = twice(lambda: ops.convert(vg, dst, out=nan_like(vg, dst), relu=relu))
        assert_bits(got, want, f"convert {src} -> {dst} n={n} relu={relu}")
        if n == 4096:       # misaligned source, misaligned destination: the scalar kernel, the same bits
            assert_bits(ops.convert(mis(vg), dst, out=nan_like(vg, dst), relu=relu), want, "convert from a misaligned source")
            assert_bits(ops.convert(vg, dst, out=mis(nan_like(vg, dst)), relu=relu), want, "convert to a misaligned destination")


def test_convert_rounds_ties_to_even():
    """The table itself, so that a reference that rounded wrongly too would show."""
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, float(np.finfo(np.float32).max), -0.0, 1 + 2.0 ** -8 + 2.0 ** -23], dtype=F32)
    got = ops.convert(gpu(v.repeat(2)[:8]), BF16).float().cpu()[:5]
    assert got.tolist() == [1.0, 1 + 2.0 ** -6, float("inf"), 0.0, 1 + 2.0 ** -7] and bool(torch.signbit(got[3]))


# ----------------------------------------------------------------------------------------------------------------------
# tanh_backward, add
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_of_w", range(6), ids=["1", "3", "1001", "4096", "grid+77", "w*(grid+300)"])
def test_tanh_backward_and_add(n_of_w):
    """tanh_backward: dx = g (1 - y y) in fp32 rounds y y (at most 2^-25 absolute, y y < 1), the difference and the product
    (2^-24 relative each): |err| <= 2^-25 |g| + 2^-23 |dx|.  The existing atol of 1e-7 covers the first term up to |g| = 3.3,
    so g is clamped to [-3, 3]; the rtol of 1e-6 covers the second with room."""
    n = lengths(4)[n_of_w]
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g).clamp_(-3.0, 3.0)
    b = torch.randn(n, generator=g)
    y = torch.tanh(torch.randn(n, generator=g) * 1.5)
    ag, bg, yg = gpu(a), gpu(b), gpu(y)
    want = (a.double() * (1.0 - y.double() * y.double())).numpy()
    got = twice(lambda: ops.tanh_backward(ag, yg, out=nan_like(yg)))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=1e-7)
    err = np.abs(got.cpu().numpy() - want)
    note("tanh_backward", float((err / (1e-7 + 1e-6 * np.abs(want))).max()), f"n={n}")
    assert_bits(twice(lambda: ops.add(ag, bg, out=nan_like(ag))), a + b, f"add n={n}")
    assert_bits(twice(lambda: ops.add(ag, None, out=nan_like(ag))), a, f"add n={n} b=None")
    if n == 4096:
        assert_bits(ops.tanh_backward(mis(ag), yg, out=nan_like(yg)), got.cpu(), "tanh_backward, misaligned g")
        assert_bits(ops.tanh_backward(ag, yg, out=mis(nan_like(yg))), got.cpu(), "tanh_backward, misaligned dx")
        assert_bits(ops.add(ag, mis(bg), out=nan_like(ag)), a + b, "add, misaligned b")
        assert_bits(ops.add(mis(ag), None, out=mis(nan_like(ag))), a, "add, misaligned a and y")


# ----------------------------------------------------------------------------------------------------------------------
# add_per_clip, clip_colsum
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,rows,C,dts", [
    (1, 1, 8, (F32, BF16)),             # one 16-byte piece (bf16) / two (fp32)
    (3, 7, 96, (F32, BF16)),            # non-power-of-two C
    (2, 5000, 128, (F32, BF16)),        # several blocks, two clips
    (3, 44001, 32, (F32, BF16)),        # fp32: 1 056 024 pieces > one grid, 352 008 per clip: the stride is no multiple of a clip
    (3, 88001, 32, (BF16,)),            # the same for bf16 output (8 channels per piece): 1 056 012 pieces
], ids=str)
def test_add_per_clip(B, rows, C, dts):
    g = torch.Generator().manual_seed(B * rows + C)
    x = torch.randn(B, rows, C, generator=g)
    r = torch.randn(B, C, generator=g)
    xg, rg = gpu(x), gpu(r)
    s = x + r[:, None, :]
    for dt in dts:
        got = twice(lambda: ops.add_per_clip(xg, rg, out=nan_like(xg, dt)))
        assert_bits(got, s.to(dt), f"add_per_clip ({B}, {rows}, {C}) -> {dt}")


def _clip_slab_start(rows):
    R = -(-rows // 16)          # CLIP_SLABS = 16
    return ((rows - 1) // R) * R


@DT
@pytest.mark.parametrize("data", ["int", "gauss"])
@pytest.mark.parametrize("B,rows,C", [
    (1, 5, 8),              # fewer rows than CLIP_SLABS: 11 empty slabs
    (5, 16, 96),            # one row per slab
    (2, 17, 1000),          # 2 rows per slab, 9 slabs used, the last with one row; fp32 CW = 250 (one row group, 6 idle threads)
    (3, 4000, 1024),        # the widest C; chain fp32: 250 rows + 1 group + 16 slabs = 267, bf16: 125 + 2 + 16
    (2, 70001, 8),          # chain fp32: 35 + 128 + 16 = 179, bf16: 18 + 256 + 16 = 290
], ids=str)
def test_clip_colsum(B, rows, C, data, dt):
    g = torch.Generator().manual_seed(B * rows + C)
    if data == "int":       # integer-valued: every fp32 partial sum is exact; non-zero at the ends of each clip and of its last slab
        x = torch.randint(-3, 4, (B, rows, C), generator=g).float()
        for k, r in enumerate(sorted({0, rows - 1, _clip_slab_start(rows)})):
            x[:, r] = torch.tensor([3.0, -2.0, 1.0, 2.0]).repeat(C // 4) * (1 if k % 2 == 0 else -1)
    else:
        x = torch.randn(B, rows, C, generator=g) + 0.5
    x = x.to(dt)
    xg = gpu(x)
    poison((B, C), F32)
    got = twice(lambda: ops.clip_colsum(xg, B))
    want = x.double().sum(1)
    if data == "int":
        assert torch.equal(got.double().cpu(), want), f"clip_colsum of integers is off by {float((got.double().cpu() - want).abs().max())}"
    else:
        within("fp32 sums", got, want, 2e-5 * x.double().abs().sum(1), f"clip_colsum ({B}, {rows}, {C}) {dt}")


# ----------------------------------------------------------------------------------------------------------------------
# codebook_grad_from_sums, increment_counters
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D", [(7, 24), (513, 128), (8192, 256)], ids=str)          # the last: 2 M elements, two grids
def test_codebook_grad_from_sums(K, D):
    g = torch.Generator().manual_seed(K + D)
    e = torch.randn(K, D, generator=g)
    n = torch.randint(0, 50, (K,), generator=g).float()
    s = torch.randn(K, D, generator=g) * 7.0
    scale = torch.tensor(0.3, dtype=F32)
    want = ((e * n[:, None]) - s) * scale          # three separately rounded fp32 operations
    eg, ng, sg = gpu(e), gpu(n), gpu(s)
    got = twice(lambda: ops.codebook_grad_from_sums(eg, ng, sg, float(scale), nan_like(eg)))
    assert_bits(got, want, f"codebook_grad_from_sums ({K}, {D})")


@pytest.mark.parametrize("n", [0, 1, 32, 33, 70])          # 32 pointers per launch: 33 and 70 take two and three
def test_increment_counters(n):
    buf = torch.arange(2 * n + 2, dtype=torch.int64, device=DEV) * 1000
    before = buf.clone()
    counters = [buf[2 * i:2 * i + 1] for i in range(n)]          # every other element: the ones between must stay
    ops.increment_counters(counters)
    ops.increment_counters(counters)
    want = before.clone()
    want[0:2 * n:2] += 2
    assert torch.equal(buf, want)


# ----------------------------------------------------------------------------------------------------------------------
# adam_step
# ----------------------------------------------------------------------------------------------------------------------
ADAM_STEPS = (1, 2, 3, 10000)


def _adam_check(n, grad_scale, view):
    """Each step on its own: the fp64 reference starts from the kernel's fp32 p, m, v of the step before.
    Gradients: magnitude 10^-1 .. 10^-6 (log-uniform, fresh each step), ONE sign per element for all steps.  Then m and g never
    cancel and the 4 * 2^-24 of m follows: m' = m + (g - m)(1 - b1) rounds g - m, the product and the sum, at most
    2^-24 (0.2 |g - m| + |m'|), and with equal signs |m'| >= 0.1 |g - m| (g > m) or >= 0.9 |g - m| (g < m).  v' = v b2 + g g (1 - b2)
    has positive terms only: 4 roundings of at most 2^-24 relative, two of them on the small term."""
    lr, b1, b2, eps = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))          # as the C ABI receives them
    g = torch.Generator().manual_seed(n + int(100 * grad_scale))
    p = gpu(torch.randn(n, generator=g) * 1.1)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    if view:
        p, m, v = mis(p), mis(m), mis(v)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    for step in ADAM_STEPS:
        grad = sign * 10.0 ** (-1.0 - 5.0 * torch.rand(n, generator=g))
        gin = gpu(grad / grad_scale)          # (1 and 0.25: exact)
        p0, m0, v0 = p.double().cpu(), m.double().cpu(), v.double().cpu()
        ops.adam_step(p, mis(gin) if view else gin, m, v, step, grad_scale=grad_scale)
        gs = gin.double().cpu() * grad_scale
        m64 = m0 + (gs - m0) * (1.0 - b1)
        v64 = v0 * b2 + gs * gs * (1.0 - b2)
        what = f"adam n={n} step={step} grad_scale={grad_scale}"
        within("adam m, v", m, m64, 4 * U32 * m64.abs() + TINY32, what + " m")
        within("adam m, v", v, v64, 4 * U32 * v64.abs() + TINY32, what + " v")
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        upd64 = (lr / bc1) * m64 / (v64.sqrt() / bc2 ** 0.5 + eps)
        p64 = p0 - upd64
        within("adam p", p, p64, U32 * p64.abs() + 8 * U32 * upd64.abs(), what + " p")
        # the parameter update alone, from the m', v' the kernel stored and used: sqrt, two quotients, the sum with eps, the
        # product, and the fp32 roundings of lr / bc1 and sqrt(bc2): 7 roundings
        upd_k = (lr / bc1) * m.double().cpu() / (v.double().cpu().sqrt() / bc2 ** 0.5 + eps)
        within("adam p (update from the stored m', v')", p, p0 - upd_k, U32 * (p0 - upd_k).abs() + 8 * U32 * upd_k.abs(), what + " p | m', v'")


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("n,view", [(1, False), (3, False), (5000, False), (5003, False), (5000, True), (4 * (GRID + 300), False)],
                         ids=["1", "3", "5000", "5003", "5000-misaligned", "4*(grid+300)"])
def test_adam_step(n, view, grad_scale):
    """n = 1, 3, 5003: scalar kernel; 5000: float4 kernel; a misaligned view of 5000: scalar again; 4 (GRID + 300): float4 with
    a grid stride, |p| up to 5 (the existing test's atol of 2e-7 is for 5000 parameters of size 1 and stays there)."""
    _adam_check(n, grad_scale, view)


def test_adam_misaligned_view_gives_the_aligned_bits():
    n = 5000
    g = torch.Generator().manual_seed(5)
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    res = []
    for view in (False, True):
        f = mis if view else (lambda t: t)
        p, m, v, gg = f(gpu(p0)), f(torch.zeros(n, device=DEV)), f(torch.zeros(n, device=DEV)), f(gpu(grad))
        for step in (1, 2):
            ops.adam_step(p, gg, m, v, step)
        res.append((p.cpu(), m.cpu(), v.cpu()))
    for a, b in zip(*res):
        assert_bits(a, b, "adam on a misaligned view")


# ----------------------------------------------------------------------------------------------------------------------
# mse_padded, vq_losses
# ----------------------------------------------------------------------------------------------------------------------
def _grad_bound(want_terms, d_operands, scale64):
    """4 * 2^-24 of the terms' magnitudes (the scale's own rounding, the product, the sum) + the rounding of d = a - c, at most
    2^-24 max(|a|, |c|), times the scale."""
    return 4 * U32 * want_terms + U32 * d_operands * abs(scale64)


@pytest.mark.parametrize("data", ["uniform", "int"])
@pytest.mark.parametrize("rows,wa,wc", [
    (1, 1, 1),                  # one element
    (160, 28, 31),              # padded, several blocks
    (160, 64, 64),              # wa == wc: nothing to pad
    (6, 1020, 1023),            # wide rows
    (300, 1000, 1023),          # 306 900 elements > 1024 * 256: the block count is capped, the loop strides
], ids=str)
def test_mse_padded(rows, wa, wc, data):
    g = torch.Generator().manual_seed(rows + wa)
    if data == "int":
        a = torch.randint(-3, 4, (rows, wa), generator=g).float()
        c = torch.randint(-3, 4, (rows, wc), generator=g).float()
    else:
        a, c = torch.rand(rows, wa, generator=g), torch.rand(rows, wc, generator=g)
    n = rows * wc
    pad = torch.zeros(rows, wc, dtype=torch.float64)
    pad[:, :wa] = a.double()
    d = pad - c.double()
    S = float((d * d).sum())
    ag, cg = gpu(a), gpu(c)
    poison(a.shape, F32)
    loss, da = twice(lambda: ops.mse_padded(ag, cg, rows, wa, wc, grad_scale=0.5))
    loss2, none = ops.mse_padded(ag, cg, rows, wa, wc, grad_scale=0.5, want_grad=False)
    assert none is None and torch.equal(loss2, loss)
    what = f"mse_padded ({rows}, {wa}, {wc}) {data}"
    if data == "int":       # d, d * d and the double sum are exact
        assert loss.item() == float(np.float32(S / n)), f"{what}: loss {loss.item()!r} vs {float(np.float32(S / n))!r}"
    np.testing.assert_allclose(loss.item(), S / n, rtol=1e-6)
    note("losses", abs(loss.item() - S / n) / (1e-6 * S / n) if S else 0.0, what)
    gs = 0.5 * 2.0 / n
    want = gs * d[:, :wa]
    within("loss gradients", da, want, _grad_bound(want.abs(), torch.maximum(a.double().abs(), c.double()[:, :wa].abs()), gs), what + " da")


@pytest.mark.parametrize("data", ["gauss", "int"])
@pytest.mark.parametrize("dt,with_add,want_dz,want_dq", [(F32, True, True, True), (BF16, True, True, True), (F32, False, True, False),
                                                         (BF16, False, False, True), (F32, False, False, False)],
                         ids=["f32-add", "bf16-add", "f32-dz_only", "bf16-dq_only", "loss_only"])
@pytest.mark.parametrize("n", [8 * 1000, 8 * 1000 + 3, 8 * (RED + 300), 8 * (RED + 300) + 3],
                         ids=["8k", "8k+3", "8(red+300)", "8(red+300)+3"])
def test_vq_losses(n, dt, with_add, want_dz, want_dq, data):
    """n = 8 k: 8 elements per thread; 8 k + 3: the scalar kernel; above 8 * 262 144 (vector) or 262 144 (scalar) elements the
    block count is capped at 1024 and the loop strides."""
    g = torch.Generator().manual_seed(n)
    if data == "int":
        z = torch.randint(-3, 4, (n,), generator=g).float()
        q = torch.randint(-3, 4, (n,), generator=g).float()
    else:
        z, q = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    add = (torch.randn(n, generator=g) * 1e-6).to(dt) if with_add else None
    zg, qg, addg = gpu(z), gpu(q), gpu(add) if with_add else None
    poison((n,), dt)
    poison((n,), F32)
    loss, dz, dq = twice(lambda: ops.vq_losses(zg, qg, dz_scale=0.25, dq_scale=1.0, dz_add=addg, want_dz=want_dz, want_dq=want_dq,
                                               grad_dtype=dt))
    assert (dz is None) == (not want_dz) and (dq is None) == (not want_dq)
    d = z.double() - q.double()
    S = float((d * d).sum())
    what = f"vq_losses n={n} {dt} {data}"
    if data == "int":
        assert loss.item() == float(np.float32(S / n)), f"{what}: loss {loss.item()!r} vs {float(np.float32(S / n))!r}"
    np.testing.assert_allclose(loss.item(), S / n, rtol=1e-6)
    note("losses", abs(loss.item() - S / n) / (1e-6 * S / n), what)
    dmax = torch.maximum(z.double().abs(), q.double().abs())
    if want_dz:
        zs = 0.25 * 2.0 / n
        a64 = add.double() if with_add else torch.zeros(1, dtype=torch.float64)
        want = d * zs + a64
        bound = _grad_bound((d * zs).abs() + a64.abs(), dmax, zs)
        assert dz.dtype == dt
        within("loss gradients" + (" (bf16)" if dt == BF16 else ""), dz, want, bound + (BF16_HALF_ULP * want.abs() if dt == BF16 else 0.0), what + " dz")
    if want_dq:
        qs = 2.0 / n
        want = d * -qs
        assert dq.dtype == F32
        within("loss gradients", dq, want, _grad_bound(want.abs(), dmax, qs), what + " dq")


def test_vq_losses_misaligned():
    """A misaligned z sends the call down the scalar kernel: the same loss partial order is not promised, the values are."""
    n = 8000
    g = torch.Generator().manual_seed(3)
    z, q = torch.randint(-3, 4, (n,), generator=g).float(), torch.randint(-3, 4, (n,), generator=g).float()
    l0, dz0, dq0 = ops.vq_losses(gpu(z), gpu(q))
    l1, dz1, dq1 = ops.vq_losses(mis(gpu(z)), gpu(q))
    assert torch.equal(l0, l1)          # integer operands: the loss is exact on either path
    assert_bits(dz1, dz0.cpu(), "vq_losses dz, misaligned z")
    assert_bits(dq1, dq0.cpu(), "vq_losses dq, misaligned z")


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[elementwise envelope] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
