"""The BatchNorm kernels (csrc/bn.hip) over their envelope, each against the fp64 yardstick tests/helpers/bn_ref64.py: both
storage types, the row counts at which slab_geom, the finalisers' chunks and bn_apply's grid stride take another path, the
channel counts that leave threads idle, and the columns on which a variance formula goes wrong.

Every kernel is checked in isolation: bn_apply and bn_backward are handed the fp32 mean / invstd that ops.bn_stats returned and
the reference takes exactly those, widened; bn_stats itself is compared with the fp64 statistics.  References take the operands
as the kernel sees them (bf16 inputs rounded first, then widened).

Bounds (none is tuned against the kernels):
  outputs stored fp32      forward 1e-5 of scale, dx 3e-5 of scale, mean rtol 1e-5 + atol (2e-6 std + 1e-6), invstd rtol 2e-5,
                           running statistics rtol 1e-5 + atol 1e-6          (test_batchnorm_train_forward_backward's figures)
  outputs stored bf16      one rounding more: |got - want| <= 2^-8 |want| + (the fp32 figure) * scale
  fp32 sums                |got - want| <= 2e-5 * sum |term| over the column: the longest chain of fp32 additions in these kernels
                           is a thread's share of a slab plus at most 256 row groups, kept below 300 (300 * 2^-24 = 1.8e-5) --
                           bn_ref64.CASES says the chain of each case, test_bn_ref_host.py asserts it.  dx_colsum adds the
                           roundings of the fp32 dx it sums, 8 * 2^-24 of the magnitudes dx is formed from (see the assertion)
  integer probe            dbeta equals the fp64 sum exactly, mean within 4 * 2^-24 * max |x|: a lost or doubled row of 70 001
                           is far inside the 2e-5 bound above, and far outside these
  fragile ReLU decisions   bn_ref64.fragile: left out of the per-element dx comparison, their terms added to the sums' bounds; more
                           than max(4, 1e-5 numel) of them fail the test"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from neural_sound_generation_amd._lib import NsgError  # noqa: E402
from tests.helpers import bn_ref64 as R  # noqa: E402

DEV = "cuda:0"
BF16_HALF_ULP = 2.0 ** -8
WORST = {}          # tolerance class -> (largest error / bound seen, where)


def gpu(t):
    return t.to(DEV).contiguous()


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _within(cls, got, want, bound, what, skip=None):
    """|got - want| <= bound element by element (bound: a float or a tensor of want's shape); prints nothing, records the
    largest err / bound of its class."""
    err = (got.detach().double().cpu() - want).abs()
    if skip is not None:
        err = torch.where(skip, torch.zeros_like(err), err)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    _note(cls, ratio, what)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def _stored(cls, got, want, tol, what, skip=None, scale=None):
    """An element-wise output against fp64: tol * scale when stored fp32, one bf16 rounding more when stored bf16."""
    scale = max(float(want.abs().max()), 1e-6) if scale is None else scale
    if got.dtype == torch.bfloat16:
        _within(cls + " (bf16)", got, want, BF16_HALF_ULP * want.abs() + tol * scale, what, skip)
    else:
        _within(cls + " (fp32)", got, want, tol * scale, what, skip)


def _poison(like):
    """The next torch.empty of this size is most likely handed this block: an output element the kernel does not write then
    reads NaN, not the right value a freed earlier result left there."""
    t = torch.full(like.shape, float("nan"), dtype=like.dtype, device=like.device)
    del t


def _twice(fn):
    a = fn()
    b = fn()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(u, v), "two runs of the same call differ"
    return a


# ----------------------------------------------------------------------------------------------------------------------
# the cases of bn_ref64.CASES, each with Gaussian data and with the integer probe
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=R.case_ids(), ids=lambda p: f"{p[0]}x{p[1]}-{p[2]}-{p[3]}")
def case(request):
    M, C, dt, data = request.param
    d = R.make_inputs(M, C, dt, data)
    c = types.SimpleNamespace(M=M, C=C, dt=dt, data=data, tag=f"({M}, {C}) {dt} {data}", big=M * C > (1 << 20), **d)
    c.xg, c.dyg, c.resg = gpu(c.x), gpu(c.dy), gpu(c.res)
    c.gammag, c.betag = gpu(c.gamma), gpu(c.beta)
    # the fp32 statistics every later kernel is handed (test_bn_stats checks them)
    c.mean, c.invstd = ops.bn_stats(c.xg, C)
    return c


def test_bn_stats(case):
    c = case
    mean64, invstd64, (rm64, rv64) = R.stats(c.x, running=(c.rm, c.rv))
    mean, invstd = _twice(lambda: ops.bn_stats(c.xg, c.C))
    assert torch.equal(mean, c.mean) and torch.equal(invstd, c.invstd)

    def with_running():
        rm, rv = gpu(c.rm), gpu(c.rv)
        m, i = ops.bn_stats(c.xg, c.C, rm, rv)
        return m, i, rm, rv
    m2, i2, rm, rv = _twice(with_running)
    assert torch.equal(m2, mean) and torch.equal(i2, invstd)          # the running statistics do not touch the batch's
    std64 = 1.0 / invstd64
    _within("mean", mean, mean64, 1e-5 * mean64.abs() + 2e-6 * std64 + 1e-6, c.tag + " mean")
    _within("invstd", invstd, invstd64, 2e-5 * invstd64, c.tag + " invstd")
    _within("running statistics", rm, rm64, 1e-5 * rm64.abs() + 1e-6, c.tag + " running_mean")
    _within("running statistics", rv, rv64, 1e-5 * rv64.abs() + 1e-6, c.tag + " running_var")
    if c.data == "int":
        _within("integer probe: mean", mean, mean64, 4.0 * R.U32 * float(c.x.double().abs().max()), c.tag + " mean of integers")
    if c.M == 1:        # the single-row convention: the row itself (invstd = 1/sqrt(eps) is inside the rtol above)
        assert torch.equal(mean.cpu(), c.x[0].float())


# (relu, residual, relu_residual, relu_out): every flag is on in at least one combination; the cases beyond 2^20 elements run two
APPLY_FLAGS = [(False, False, False, False), (True, False, False, False), (False, True, False, False), (True, True, True, False),
               (False, True, False, True)]
APPLY_FLAGS_BIG = [(True, True, True, False), (False, True, False, True)]


def test_bn_apply(case):
    c = case
    for relu, res, relu_res, relu_out in (APPLY_FLAGS_BIG if c.big else APPLY_FLAGS):
        out = torch.full((c.M, c.C), float("nan"), dtype=c.xg.dtype, device=DEV)
        y = _twice(lambda: ops.bn_apply(c.xg, c.mean, c.invstd, c.gammag, c.betag, relu=relu, residual=c.resg if res else None,
                                        relu_residual=relu_res, relu_out=relu_out, out=out).clone())
        want = R.apply(c.x, c.mean, c.invstd, c.gamma, c.beta, relu=relu, residual=c.res if res else None,
                       relu_residual=relu_res, relu_out=relu_out)
        _stored("forward", y, want, 1e-5, f"{c.tag} bn_apply relu={relu} res={res} relu_res={relu_res} relu_out={relu_out}")
        if relu and not res or relu_out:
            assert float(y.float().min()) >= 0.0


def _backward(c, form, colsum=True):
    kw = {}
    if form == "yrelu":
        kw["y_relu"] = c.yrelu
    elif form == "beta":
        kw["relu_beta"] = c.betag
    nan = float("nan")
    cs = torch.full((c.C,), nan, device=DEV) if colsum else None
    dx, dg, db = ops.bn_backward(c.xg, kw.get("y_relu"), c.dyg, c.mean, c.invstd, c.gammag, relu_beta=kw.get("relu_beta"), dx_colsum=cs,
                                 out=torch.full((c.M, c.C), nan, dtype=c.xg.dtype, device=DEV), dgamma=torch.full((c.C,), nan, device=DEV),
                                 dbeta=torch.full((c.C,), nan, device=DEV))
    return (dx, dg, db, cs) if colsum else (dx, dg, db)


def test_bn_backward(case):
    c = case
    c.yrelu = ops.bn_apply(c.xg, c.mean, c.invstd, c.gammag, c.betag, relu=True)
    res = {form: _twice(lambda: _backward(c, form)) for form in ("yrelu", "beta", "none")}
    # the mask re-derived from x is the forward's own expression: the stored output's mask, bit for bit
    for a, b in zip(res["yrelu"], res["beta"]):
        assert torch.equal(a, b), "mask from y_relu and mask from relu_beta disagree"
    # without the column sums: the same dx, dgamma, dbeta
    for a, b in zip(_backward(c, "none", colsum=False), res["none"][:3]):
        assert torch.equal(a, b)
    # the two halves equal the whole, bit for bit
    for form, rb in (("beta", c.betag), ("none", None)):
        dx, dg, db, cs = res[form]
        dg2, db2 = _twice(lambda: ops.bn_backward_sums(c.xg, c.dyg, c.mean, c.invstd, c.gammag, relu_beta=rb,
                                                       dgamma=torch.full((c.C,), float("nan"), device=DEV),
                                                       dbeta=torch.full((c.C,), float("nan"), device=DEV)))
        assert torch.equal(dg2, dg) and torch.equal(db2, db)
        cs2 = torch.full((c.C,), float("nan"), device=DEV)
        _poison(dx)
        dx2 = ops.bn_backward_apply(c.xg, c.dyg, c.mean, c.invstd, c.gammag, dg2, db2, relu_beta=rb, dx_colsum=cs2)
        assert torch.equal(dx2, dx) and torch.equal(cs2, cs)
        _poison(dx)
        assert torch.equal(ops.bn_backward_apply(c.xg, c.dyg, c.mean, c.invstd, c.gammag, dg2, db2, relu_beta=rb), dx)

    fragile = R.fragile(c.x, c.mean, c.invstd, c.gamma, c.beta)
    nfr = int(fragile.sum())
    assert nfr <= R.fragile_cap(c.M * c.C), f"{c.tag}: {nfr} fragile ReLU decisions"
    mask64 = R.relu_mask(c.x, c.mean, c.invstd, c.gamma, c.beta)
    xhat_abs = ((c.x.double() - c.mean.double().cpu()) * c.invstd.double().cpu()).abs()
    sc_abs = (c.gamma.double() * c.invstd.double().cpu()).abs()
    for form, mask, fr in (("beta", mask64, fragile), ("none", None, None)):
        dx, dg, db, cs = res[form]
        w_dx, w_dg, w_db, w_cs = R.backward(c.x, c.dy, c.mean, c.invstd, c.gamma, mask)
        t_dg, t_db, t_cs, t_parts = R.backward_terms(c.x, c.dy, c.mean, c.invstd, c.gamma, mask, dx=w_dx)
        wide_dg = wide_db = wide_cs = 0.0
        if fr is not None and nfr:      # either decision is correct there: the terms those elements may add or withhold
            gfr = torch.where(fr, c.dy.double().abs(), torch.zeros(1, dtype=torch.float64))
            wide_db, wide_dg, wide_cs = gfr.sum(0), (gfr * xhat_abs).sum(0), sc_abs * gfr.sum(0)
        what = f"{c.tag} bn_backward mask={form}"
        _stored("dx", dx, w_dx, 3e-5, what + " dx", skip=fr)
        _within("fp32 sums", dg, w_dg, 2e-5 * t_dg + wide_dg, what + " dgamma")
        _within("fp32 sums", db, w_db, 2e-5 * t_db + wide_db, what + " dbeta")
        # dx_colsum adds up the kernel's own fp32 dx.  Each of those carries the roundings of the three magnitudes it is formed
        # from, gamma invstd (dy - dbeta / M - xhat dgamma / M): x - mean, xhat, the two means (1 / M and its product), the
        # product xhat dgamma / M, two differences, gamma invstd and the last product -- at most 8 * 2^-24 of those magnitudes,
        # which is NOT relative to |dx| where dx cancels (three rows whose dy lies in the span of 1 and xhat: dx = 1e-6 dy).
        # The first version of this bound, 2e-5 * sum |dx| alone, missed that and failed at (3, 8) and (5, 96) by 1e-7 absolute;
        # where dx does not cancel the second term is a few per cent of the first (8 * 2^-24 = 4.8e-7 against 2e-5).
        _within("fp32 sums", cs, w_cs, 2e-5 * t_cs + 8 * R.U32 * t_parts + wide_cs, what + " dx_colsum")
        if c.data == "int":         # integer-valued dy: every fp32 partial sum is exact, so is the double pooling
            exact = torch.ones(c.C, dtype=torch.bool) if fr is None else ~fr.any(0)
            got, want = db.double().cpu(), w_db
            assert torch.equal(got[exact], want[exact]), \
                f"{what}: dbeta of integers is off by {float((got - want)[exact].abs().max())} (a row lost or counted twice?)"
            _note("integer probe: dbeta", 0.0, what)
    if c.M == 1:        # dy - mean(dy) = 0 and xhat = 0
        assert float(res["none"][0].float().abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# mixed storage types of bn_apply, special columns, eval statistics, error returns
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", R.MIXED_CASES, ids=str)
@pytest.mark.parametrize("src,dst", [(R.F32, R.BF16), (R.BF16, R.F32)], ids=["f32_to_bf16", "bf16_to_f32"])
def test_bn_apply_mixed_types(M, C, src, dst):
    """x and the residual of one type, y of the other (8 channels per thread either way), with the residual and every ReLU."""
    d = R.make_inputs(M, C, src, "gauss")
    xg, resg, gammag, betag = gpu(d["x"]), gpu(d["res"]), gpu(d["gamma"]), gpu(d["beta"])
    mean, invstd = ops.bn_stats(xg, C)
    for relu, relu_res, relu_out in ((False, False, False), (True, True, False), (False, False, True)):
        out = torch.full((M, C), float("nan"), dtype=R.torch_dtype(dst), device=DEV)
        y = _twice(lambda: ops.bn_apply(xg, mean, invstd, gammag, betag, relu=relu, residual=resg, relu_residual=relu_res,
                                        relu_out=relu_out, out=out).clone())
        assert y.dtype == R.torch_dtype(dst)
        y2 = ops.bn_apply(xg, mean, invstd, gammag, betag, relu=relu, residual=resg, relu_residual=relu_res, relu_out=relu_out,
                          out_dtype=R.torch_dtype(dst))
        assert torch.equal(y2, y)
        want = R.apply(d["x"], mean, invstd, d["gamma"], d["beta"], relu=relu, residual=d["res"], relu_residual=relu_res, relu_out=relu_out)
        _stored("forward", y, want, 1e-5, f"({M}, {C}) bn_apply {src} -> {dst} relu={relu} relu_out={relu_out}")


def _per_column(cls, got, want, tol, what):
    """tol of each COLUMN's scale: one column 300 times larger than its neighbours must not hide them."""
    _within(cls + " (fp32)", got, want, tol * want.abs().amax(0).clamp_min(1e-6), what)


def test_column_whose_mean_dwarfs_its_spread():
    """x = 0.5 randn + 1000 in fp32: x^2 is 1e6 with an fp32 rounding of 0.06, the variance is 0.25 -- a variance formed as
    E[x^2] - E[x]^2 (or about a pivot of 0) is off by tens of per cent; about a sample of the column it keeps invstd's 2e-5."""
    d = R.special_inputs("offset")
    M, C = R.SPECIAL_MC
    xg = gpu(d["x"])
    mean, invstd = _twice(lambda: ops.bn_stats(xg, C))
    mean64, invstd64, _ = R.stats(d["x"])
    _within("invstd", invstd, invstd64, 2e-5 * invstd64, "offset column invstd")
    _within("mean", mean, mean64, 1e-5 * mean64.abs() + 2e-6 / invstd64 + 1e-6, "offset column mean")
    y = ops.bn_apply(xg, mean, invstd, gpu(d["gamma"]), gpu(d["beta"]), relu=True)
    _per_column("forward", y, R.apply(d["x"], mean, invstd, d["gamma"], d["beta"], relu=True), 1e-5, "offset column forward")
    dx, dg, db = ops.bn_backward(xg, None, gpu(d["dy"]), mean, invstd, gpu(d["gamma"]))
    w_dx, w_dg, w_db, _ = R.backward(d["x"], d["dy"], mean, invstd, d["gamma"])
    t_dg, t_db, _, _ = R.backward_terms(d["x"], d["dy"], mean, invstd, d["gamma"])
    _per_column("dx", dx, w_dx, 3e-5, "offset column dx")
    _within("fp32 sums", dg, w_dg, 2e-5 * t_dg, "offset column dgamma")
    _within("fp32 sums", db, w_db, 2e-5 * t_db, "offset column dbeta")


def test_constant_and_zero_columns():
    """Zero variance: mean is the constant itself, invstd = 1/sqrt(eps) to fp32's rounding, no NaN anywhere; xhat = 0 gives
    dgamma = 0 and dx = gamma invstd (dy - mean(dy)).  The neighbouring columns keep their own accuracy."""
    d = R.special_inputs("constant")
    M, C = R.SPECIAL_MC
    xg, dyg, gammag, betag = gpu(d["x"]), gpu(d["dy"]), gpu(d["gamma"]), gpu(d["beta"])
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd = _twice(lambda: ops.bn_stats(xg, C))
    m2, i2 = ops.bn_stats(xg, C, rm, rv)
    assert torch.equal(m2, mean) and torch.equal(i2, invstd)
    mean64, invstd64, (rm64, rv64) = R.stats(d["x"], running=(torch.zeros(C), torch.ones(C)))
    assert mean[:2].tolist() == [7.25, 0.0]
    _within("invstd", invstd, invstd64, 2e-5 * invstd64, "constant column invstd")
    _within("mean", mean, mean64, 1e-5 * mean64.abs() + 2e-6 / invstd64 + 1e-6, "constant column mean")
    _within("running statistics", rm, rm64, 1e-5 * rm64.abs() + 1e-6, "constant column running_mean")
    _within("running statistics", rv, rv64, 1e-5 * rv64.abs() + 1e-6, "constant column running_var")
    y = ops.bn_apply(xg, mean, invstd, gammag, betag)
    assert torch.equal(y[:, :2].cpu(), d["beta"][:2].expand(M, 2))          # (x - mean) = 0 exactly: y = beta
    _per_column("forward", y, R.apply(d["x"], mean, invstd, d["gamma"], d["beta"]), 1e-5, "constant column forward")
    for rb in (None, betag):
        dx, dg, db = _twice(lambda: ops.bn_backward(xg, None, dyg, mean, invstd, gammag, relu_beta=rb))
        mask = None if rb is None else R.relu_mask(d["x"], mean, invstd, d["gamma"], d["beta"])
        fr = None if rb is None else R.fragile(d["x"], mean, invstd, d["gamma"], d["beta"])
        assert fr is None or int(fr.sum()) <= R.fragile_cap(M * C)
        assert fr is None or not bool(fr[:, :2].any())          # t = beta in the constant columns: nothing fragile about it
        w_dx, w_dg, w_db, _ = R.backward(d["x"], d["dy"], mean, invstd, d["gamma"], mask)
        t_dg, t_db, _, _ = R.backward_terms(d["x"], d["dy"], mean, invstd, d["gamma"], mask)
        wide = 0.0 if fr is None else torch.where(fr, d["dy"].double().abs(), torch.zeros(1, dtype=torch.float64)).sum(0)
        assert dg[:2].tolist() == [0.0, 0.0]
        err = (dx.double().cpu() - w_dx).abs()
        if fr is not None:
            err = torch.where(fr, torch.zeros_like(err), err)
        ratio = float((err / (3e-5 * w_dx.abs().amax(0).clamp_min(1e-6))).max())
        _note("dx (fp32)", ratio, "constant column dx")
        assert ratio <= 1.0, f"constant column dx: error / bound = {ratio:.3f}"
        xhat = ((d["x"].double() - mean.double().cpu()) * invstd.double().cpu()).abs()
        _within("fp32 sums", dg, w_dg, 2e-5 * t_dg + wide * xhat.amax(0), "constant column dgamma")
        _within("fp32 sums", db, w_db, 2e-5 * t_db + wide, "constant column dbeta")


def test_bn_eval_stats_at_a_ragged_channel_count():
    """C = 100 is no multiple of the kernel's 64-thread block: the second block's last 28 threads write nothing."""
    g = torch.Generator().manual_seed(100)
    rm, rv = torch.randn(100, generator=g), torch.rand(100, generator=g) + 0.01
    mean, invstd = _twice(lambda: ops.bn_eval_stats(gpu(rm), gpu(rv)))
    assert torch.equal(mean.cpu(), rm)
    want = 1.0 / torch.sqrt(rv.double() + float(torch.tensor(R.EPS, dtype=torch.float32)))
    _within("invstd", invstd, want, 2e-5 * want, "bn_eval_stats invstd")


def test_unsupported_shapes_and_misaligned_pointers_are_errors():
    """Each of these is refused before anything is launched (check_mc, the alignment requirements): an error, not a fault."""
    def args(M, C, dt):
        x = torch.zeros(M, C, dtype=dt, device=DEV)
        v = torch.ones(C, device=DEV)
        return x, v

    for M, C, dt in ((16, 12, torch.bfloat16), (16, 1028, torch.float32), (16, 1028, torch.bfloat16)):
        x, v = args(M, C, dt)
        with pytest.raises(NsgError):
            ops.bn_stats(x, C)
        with pytest.raises(NsgError):
            ops.bn_apply(x, v, v, v, v)
        with pytest.raises(NsgError):
            ops.bn_backward(x, None, x, v, v, v)
        with pytest.raises(NsgError):
            ops.bn_backward_sums(x, x, v, v, v)
        with pytest.raises(NsgError):
            ops.bn_backward_apply(x, x, v, v, v, v, v)
    # fp32 -> bf16 takes 8 channels per thread: C = 12 is fine for fp32 -> fp32 and refused for the mixed pair
    x, v = args(16, 12, torch.float32)
    ops.bn_apply(x, v, v, v, v)
    with pytest.raises(NsgError):
        ops.bn_apply(x, v, v, v, v, out_dtype=torch.bfloat16)
    # a contiguous view that starts at element 1 of its buffer: not 16-byte aligned
    for dt in (torch.float32, torch.bfloat16):
        M, C = 16, 16
        x = torch.zeros(M * C + 8, dtype=dt, device=DEV)[1:1 + M * C].view(M, C)
        ok = torch.zeros(M, C, dtype=dt, device=DEV)
        v = torch.ones(C, device=DEV)
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
        with pytest.raises(NsgError):
            ops.bn_stats(x, C)
        with pytest.raises(NsgError):
            ops.bn_apply(x, v, v, v, v, out=ok)
        with pytest.raises(NsgError):
            ops.bn_apply(ok, v, v, v, v, residual=x)
        with pytest.raises(NsgError):
            ops.bn_apply(ok, v, v, v, v, out=x)
        with pytest.raises(NsgError):
            ops.bn_backward(x, None, ok, v, v, v)
        with pytest.raises(NsgError):
            ops.bn_backward(ok, None, x, v, v, v)
        with pytest.raises(NsgError):
            ops.bn_backward_sums(x, ok, v, v, v)
    torch.cuda.synchronize()


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[bn envelope] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
