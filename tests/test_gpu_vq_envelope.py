"""The vector quantiser's kernels (csrc/vq.hip, vq_bf16.hip, segsum.hip, the one-hot forms of gemm_wgrad.hip,
vq_losses_indexed_kernel of elementwise.hip) over their envelope, each against the fp64 yardstick tests/helpers/vq_ref64.py --
its module docstring derives every bound; tests/test_vq_ref_host.py shows on the CPU that the bounds hold for an honest
computation and that each acceptance rule rejects what a subtly wrong kernel would return.

Every call runs twice and must repeat bit for bit; every output is poisoned first (NaN, or an impossible index), so an element
a kernel never writes fails its check.  References take the operands as the kernel sees them; rows given as their sources are
formed on the CPU in fp32 in the header's order, so nothing here depends on nsg_bn_apply.

Tolerance classes (none is tuned against the kernels; the last test prints the largest error / bound each met):
  bf16x3 index             dist(picked) - dist(fp64 first minimum) <= bound(picked) + bound(minimum), every row judged
  bf16x3 dmin              |dmin - dist(picked)| <= bound(picked)
  integer probes           exact: the first index of the integer minimum and dmin itself (the fp32 search too); integer rows give
                           exact segment sums
  exact search             indices, distances and codes bit for bit those of oracle.vqvae_oracle.vq_indices
  code outputs             codes == e[idx] and codes_bf16 == bf16(relu?(e[idx] + clip row)) bit for bit
  segment sums             gamma(chain) * sum |term| per element, chain from the summation shape of each form; counts == bincount
  losses                   rtol 1e-6
  loss gradients           4 * 2^-24 of the terms + the rounding of d, + 2^-8 |want| when stored as bf16
  BatchNorm sums of dz     of dz AS STORED, 2e-5 * sum |term| (chains below 300 additions)
  ema                      gamma(2) of the terms for the two statistics, gamma(16) * T / nn for the codebook"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, ops  # noqa: E402
from neural_sound_generation_amd._lib import NsgError  # noqa: E402
from oracle import vqvae_oracle as O  # noqa: E402
from tests.helpers import vq_ref64 as R  # noqa: E402

DEV = "cuda:0"
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
NAN = float("nan")
WORST = {}          # tolerance class -> (largest error / bound seen, where)


def gpu(t):
    return t.to(DEV).contiguous()


def _note(cls, ratio, where):
    if ratio > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (ratio, where)


def _within(cls, got, want, bound, what):
    """|got - want| <= bound element by element; records the largest err / bound of its class."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got.detach().double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ok = err <= bound
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
    _note(cls, ratio, what)
    assert bool(ok.all()), f"{what}: error / bound = {ratio:.3f} (max abs err {float(err.max()):.3e})"


def _poison(shape, dtype):
    """The next torch.empty of this size is most likely handed this block: an output element the kernel does not write then
    reads NaN (an impossible index), not the right value a freed earlier result left there."""
    t = torch.full(tuple(shape), R.IDX_POISON if dtype == I64 else NAN, dtype=dtype, device=DEV)
    del t


def _full(shape, dtype=F32):
    return torch.full(tuple(shape), R.IDX_POISON if dtype == I64 else NAN, dtype=dtype, device=DEV)


def _twice(fn):
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v), "two runs of the same call differ"
    return a if len(a) > 1 else a[0]


def _bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    it = torch.int16 if g.dtype == BF16 else torch.int32
    assert torch.equal(g.view(it), w.view(it)), f"{what}: {int((g.view(it) != w.view(it)).sum())} elements differ in their bits"


def _sources(src):
    return ops.BnResRows(*[gpu(t) for t in src])


# ----------------------------------------------------------------------------------------------------------------------
# the bf16x3 search
# ----------------------------------------------------------------------------------------------------------------------
def _raw_bf16x3(x, e, idx, codes, dmin, lp, relu, clip_rows, rpc):
    """nsg_vq_forward_bf16x3_cond on caller-owned (poisoned) outputs."""
    N, D = x.shape
    K = e.shape[0]
    ws, nb = ops._ws(e.device, "nsg_vq_bf16x3_workspace_bytes", N, D, K)
    _lib.call("nsg_vq_forward_bf16x3_cond", ops._p(x), ops._p(e), N, D, K, ops._p(idx), ops._p(codes), ops._p(dmin), ops._p(lp), 1 if relu else 0,
              ops._p(clip_rows), rpc, ops._p(ws), nb, ops._stream())


def _raw_bf16x3_bnres(src, e, idx, lp, relu, clip_rows, rpc):
    """nsg_vq_forward_bf16x3_bnres itself: the widths ops.BnResRows' three-consumer rule leaves out (D % 8 == 0 is the kernel's)."""
    N, D = src.h.shape
    K = e.shape[0]
    ws, nb = ops._ws(e.device, "nsg_vq_bf16x3_workspace_bytes", N, D, K)
    _lib.call("nsg_vq_forward_bf16x3_bnres", *src.pointers(), ops._p(e), N, D, K, ops._p(idx), ops._p(None), ops._p(lp), 1 if relu else 0,
              ops._p(clip_rows), rpc, ops._p(ws), nb, ops._stream())


def _search_on_sources(src, e, mode, clip_rows=None):
    N, D = src.h.shape
    if ops.bnres_rows_supported(D):
        _poison((N,), I64)
        _poison((N, D), BF16)
        idx, _, _, lp = ops.vq_forward(src, e, want_codes=False, impl="bf16x3", codes_bf16=mode, clip_rows=clip_rows)
        return idx, lp
    idx, lp = _full((N,), I64), _full((N, D), BF16)
    _raw_bf16x3_bnres(src, e, idx, lp, mode == "relu", clip_rows, N // clip_rows.shape[0] if clip_rows is not None else 0)
    return idx, lp


def _judge(c, name, ref, x, e, planted, idx, dmin, what):
    """The acceptance rule on every row, the planted codes, and exactness on the integer probe."""
    bad = R.search_violations(ref, idx, dmin)
    r_idx, r_d = R.search_ratio(ref, idx, dmin)
    _note("bf16x3 index" if "fp32 search" not in what else "exact search (split bound)", r_idx, what)
    if dmin is not None:
        _note("bf16x3 dmin" if "fp32 search" not in what else "exact search dmin (split bound)", r_d, what)
    first = int(bad.nonzero()[0]) if bool(bad.any()) else -1
    assert int(bad.sum()) == R.SEARCH_ROWS_LEFT_OUT, f"{what}: {int(bad.sum())} rows rejected (index excess / slack {r_idx:.3f}, dmin {r_d:.3f}), first {first}"
    got = idx.cpu()
    for k, (row, code) in planted.items():
        assert int(got[row]) == code, f"{what}: planted '{k}': row {row} took code {int(got[row])}, not {code}"
    if c.data == "int":
        wrong = R.int_violations(x, e, idx, dmin)
        assert not bool(wrong.any()), f"{what}: integer probe: {int(wrong.sum())} rows are not the exact first minimum"
        _note("integer probes", 0.0, what)


@pytest.fixture(scope="module", params=R.SEARCH_CASES, ids=R.search_case_id)
def scase(request):
    N, K, D, data = request.param
    c = R.make_search_inputs(N, K, D, data)
    c.tag = R.search_case_id(request.param)
    c.ref_x, c.ref_z = R.search_ref(c.x, c.e_x), R.search_ref(c.z, c.e_z)
    c.xg, c.exg, c.ezg, c.zg = gpu(c.x), gpu(c.e_x), gpu(c.e_z), gpu(c.z)
    return c


def test_bf16x3_with_distances(scase):
    """want_dist=True: vq_forward_bf16x3_kernel<NKS, HAS_X2 = true>, with the fp32 code gather."""
    c = scase

    def run(impl):
        _poison((c.N,), I64)
        _poison((c.N, c.D), F32)
        _poison((c.N,), F32)
        return ops.vq_forward(c.xg, c.exg, want_codes=True, want_dist=True, impl=impl)
    idx, codes, dmin = _twice(lambda: run("bf16x3"))
    _judge(c, "x", c.ref_x, c.x, c.e_x, c.planted_x, idx, dmin, f"{c.tag} with distances")
    _bits(codes, c.e_x[idx.cpu()], f"{c.tag} codes")
    if c.data == "int":         # the fp32 search is exact on the probe too
        idx, codes, dmin = _twice(lambda: run("mfma"))
        _judge(c, "x", c.ref_x, c.x, c.e_x, c.planted_x, idx, dmin, f"{c.tag} fp32 search")
        _bits(codes, c.e_x[idx.cpu()], f"{c.tag} fp32 search codes")


def test_bf16x3_production_form(scase):
    """No fp32 codes, no distances, a bf16 code output: vq_forward_bf16x3_kernel<NKS, HAS_X2 = false, BNRES = false>."""
    c = scase
    seen = []
    for mode in ("plain", "relu"):
        def run():
            _poison((c.N,), I64)
            _poison((c.N, c.D), BF16)
            return ops.vq_forward(c.xg, c.exg, want_codes=False, impl="bf16x3", codes_bf16=mode)
        idx, codes, dmin, lp = _twice(run)
        assert codes is None and dmin is None
        _judge(c, "x", c.ref_x, c.x, c.e_x, c.planted_x, idx, None, f"{c.tag} production form ({mode})")
        _bits(lp, R.codes_bf16_ref(c.e_x, idx, relu=mode == "relu"), f"{c.tag} codes_bf16 ({mode})")
        seen.append(idx)
    assert torch.equal(seen[0], seen[1])


def test_bf16x3_on_sources(scase):
    """The production form on ops.BnResRows: <NKS, false, BNRES = true>; the rows are the fp32 z formed on the CPU."""
    c = scase
    src = _sources(c.src)
    for mode in ("relu", "plain"):
        idx, lp = _twice(lambda: _search_on_sources(src, c.ezg, mode))
        _judge(c, "z", c.ref_z, c.z, c.e_z, c.planted_z, idx, None, f"{c.tag} on sources ({mode})")
        _bits(lp, R.codes_bf16_ref(c.e_z, idx, relu=mode == "relu"), f"{c.tag} codes_bf16 on sources ({mode})")
    # the existing relation: bit for bit the search on the materialised rows
    idx2, _, _, lp2 = ops.vq_forward(c.zg, c.ezg, want_codes=False, impl="bf16x3", codes_bf16="plain")
    assert torch.equal(idx2, idx) and torch.equal(lp2, lp)


@pytest.mark.parametrize("rpc,clips", R.CLIP_CASES, ids=lambda v: str(v))
def test_clip_rows(rpc, clips):
    """rows_per_clip = 50 / 128 / 129: a 128-row block spans three clips, is one clip, has the clip boundary one row into the
    next block.  All three forms, plain and ReLU'd."""
    N, K, D = rpc * clips, 100, 64
    c = R.make_search_inputs(N, K, D, "gauss")
    c.data = "gauss"
    ref_x, ref_z = R.search_ref(c.x, c.e_x), R.search_ref(c.z, c.e_z)
    rows = torch.randn(clips, D, generator=torch.Generator().manual_seed(rpc)) * 0.3
    rowsg, xg, exg, ezg, src = gpu(rows), gpu(c.x), gpu(c.e_x), gpu(c.e_z), _sources(c.src)
    for mode in ("plain", "relu"):
        relu = mode == "relu"
        what = f"clip rows {rpc} x {clips} ({mode})"

        def run(dist):
            _poison((N,), I64)
            _poison((N, D), BF16)
            return ops.vq_forward(xg, exg, want_codes=False, want_dist=dist, impl="bf16x3", codes_bf16=mode, clip_rows=rowsg)
        idx, _, _, lp = _twice(lambda: run(False))
        _judge(c, "x", ref_x, c.x, c.e_x, c.planted_x, idx, None, what)
        _bits(lp, R.codes_bf16_ref(c.e_x, idx, rows, rpc, relu), what + " codes_bf16")
        idx, _, dmin, lp = _twice(lambda: run(True))
        _judge(c, "x", ref_x, c.x, c.e_x, c.planted_x, idx, dmin, what + " with distances")
        _bits(lp, R.codes_bf16_ref(c.e_x, idx, rows, rpc, relu), what + " codes_bf16 with distances")
        idx, lp = _twice(lambda: _search_on_sources(src, ezg, mode, rowsg))
        _judge(c, "z", ref_z, c.z, c.e_z, c.planted_z, idx, None, what + " on sources")
        _bits(lp, R.codes_bf16_ref(c.e_z, idx, rows, rpc, relu), what + " codes_bf16 on sources")


# ----------------------------------------------------------------------------------------------------------------------
# the exact search: slices
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K,S,why", R.EXACT_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_exact_search_slices(N, D, K, S, why):
    """S = 2, 4, 8 slices at 130 rows, ragged last slices and tiles, duplicate nearest codes in different slices (the lower index
    wins: vq_combine_kernel's strict <), K = 1, odd widths: everything bit for bit the oracle's."""
    assert R.vq_slices(N, D, K) == S
    x, e, must = R.make_exact_inputs(N, D, K, S)
    want, wdist = O.vq_indices(x, e, return_dist=True)
    xg, eg = gpu(torch.from_numpy(x)), gpu(torch.from_numpy(e))

    def run():
        _poison((N,), I64)
        _poison((N, D), F32)
        _poison((N,), F32)
        return ops.vq_forward(xg, eg, want_dist=True)
    idx, codes, dmin = _twice(run)
    assert np.array_equal(idx.cpu().numpy(), want), f"{int((idx.cpu().numpy() != want).sum())} indices differ from the oracle"
    assert np.array_equal(dmin.cpu().numpy(), wdist)
    assert np.array_equal(codes.cpu().numpy(), e[want])
    for row, a in must.items():
        assert int(idx[row]) == a, f"row {row}: duplicates in different slices resolved to {int(idx[row])}, not {a}"
    _note("exact search", 0.0, f"({N}, {D}, {K}) S={S}")


# ----------------------------------------------------------------------------------------------------------------------
# segment sums
# ----------------------------------------------------------------------------------------------------------------------
def _raw_sorted_bnres(idx, src, K, out, counts):
    N, D = src.h.shape
    ws, nb = ops._ws(out.device, "nsg_index_add_sorted_workspace_bytes", N, D, K)
    _lib.call("nsg_index_add_rows_sorted_bnres", ops._p(idx), *src.pointers(), N, D, K, ops._p(out), ops._p(counts), ops._p(ws), nb, ops._stream())


@pytest.fixture(scope="module", params=R.SEG_CASES, ids=R.seg_case_id)
def segcase(request):
    d = R.make_seg_inputs(*request.param)
    d.tag = R.seg_case_id(request.param)
    d.ref = R.seg_ref(d.idx, d.g, d.K)
    d.idxg, d.gg = gpu(d.idx), gpu(d.g)
    return d


def _check_sums(d, impl, ref, out, counts, what):
    exact = d.data == "int"
    assert torch.equal(counts.cpu().double(), ref.counts.double()), f"{what}: counts differ from bincount at {int((counts.cpu().double() != ref.counts.double()).sum())} codes"
    if exact:
        got = out.cpu().double()
        assert torch.equal(got, ref.sums), f"{what}: integer rows, {int((got != ref.sums).sum())} sums are not exact (largest difference {float((got - ref.sums).abs().max())})"
        _note("integer probes", 0.0, what)
    else:
        _within("segment sums " + impl, out, ref.sums, R.seg_bound(impl, ref), what)
    if d.kind == "oob_all":
        assert not bool(out.any()) and not bool(counts.any())


@pytest.mark.parametrize("impl", ["sorted", "f32", "bf16x2"])
def test_segment_sums(segcase, impl):
    """Gaussian rows within the chain bound, integer rows exactly, counts == bincount; rows whose index lies outside [0, K) --
    -1, K, K + 5, 2^32 + 3, -2^32 + 1, 2^32 -- contribute to neither, in every form."""
    d = segcase
    assert ops.index_add_sorted_supported(d.N, d.D, d.K)          # (or impl="sorted" would quietly run the one-hot form)

    def run():
        out, counts = _full((d.K, d.D)), _full((d.K,))
        ops.index_add_rows(d.idxg, d.gg, d.K, impl=impl, out=out, counts=counts)
        return out, counts
    out, counts = _twice(run)
    _check_sums(d, impl, d.ref, out, counts, f"{d.tag} {impl}")
    # without the counts: the same sums
    out2 = _full((d.K, d.D))
    ops.index_add_rows(d.idxg, d.gg, d.K, impl=impl, out=out2)
    assert torch.equal(out2, out)


def test_segment_sums_on_sources(segcase):
    d = segcase
    if not R.bnres_sorted_supported(d.D):
        assert d.D == 512          # the one width of the table outside the documented range of the _bnres form
        return
    src, ref = _sources(d.src), R.seg_ref(d.idx, d.z, d.K)

    def run():
        out, counts = _full((d.K, d.D)), _full((d.K,))
        if ops.bnres_rows_supported(d.D):
            ops.index_add_rows(d.idxg, src, d.K, impl="sorted", out=out, counts=counts)
        else:
            _raw_sorted_bnres(d.idxg, src, d.K, out, counts)          # D = 4: documented for this entry point, below BnResRows' rule
        return out, counts
    out, counts = _twice(run)
    _check_sums(d, "sorted_bnres", ref, out, counts, f"{d.tag} sorted on sources")
    # the existing relation: bit for bit the sums of the materialised rows
    out2 = _full((d.K, d.D))
    ops.index_add_rows(d.idxg, gpu(d.z), d.K, impl="sorted", out=out2)
    assert torch.equal(out2, out)


def test_sorted_form_refuses_d_260():
    """One rule in the header, the C check and ops.index_add_sorted_supported: widths above 256 are multiples of 256."""
    N, K = 64, 8
    for D, ok in ((260, False), (384, False), (12, False), (256, True), (768, True)):
        assert bool(ops.index_add_sorted_supported(N, D, K)) == ok == R.sorted_supported(N, D, K)
        g = torch.Generator().manual_seed(D)
        rows, idx = torch.randn(N, D, generator=g), torch.randint(0, K, (N,), generator=g)
        out, counts = _full((K, D)), _full((K,))
        ws, nb = ops._ws(out.device, "nsg_index_add_sorted_workspace_bytes", N, D, K)
        args = (ops._p(gpu(idx)), ops._p(gpu(rows)), N, D, K, ops._p(out), ops._p(counts), ops._p(ws), nb, ops._stream())
        if ok:
            _lib.call("nsg_index_add_rows_sorted", *args)
            ref = R.seg_ref(idx, rows, K)
            _within("segment sums sorted", out, ref.sums, R.seg_bound("sorted", ref), f"sorted D={D}")
        else:
            with pytest.raises(NsgError):
                _lib.call("nsg_index_add_rows_sorted", *args)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and bool(torch.isnan(counts).all())


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
def _raw_losses_bnres(src, e, idx, dz_scale, dz_add, loss, dz, dgamma, dbeta):
    N, D = src.h.shape
    ws, nb = ops._ws(e.device, "nsg_vq_losses_indexed_bn_workspace_bytes", N, D)
    _lib.call("nsg_vq_losses_indexed_bnres", *src.pointers(), ops._p(e), ops._p(idx), N, D, e.shape[0], dz_scale, ops._p(dz_add), ops._p(loss), ops._p(dz),
              ops._p(dgamma), ops._p(dbeta), ops._p(ws), nb, ops._stream())


def _losses_on_sources(src, e, idx, dz_scale, dz_add):
    N, D = src.h.shape
    if ops.bnres_rows_supported(D):
        _poison((N, D), BF16)
        return ops.vq_losses_indexed(src, e, idx, dz_scale=dz_scale, dz_add=dz_add, grad_dtype=BF16, bn=(src.h, src.mean, src.invstd),
                                     dgamma=_full((D,)), dbeta=_full((D,)))
    loss, dz, dg, db = _full((1,)), _full((N, D), BF16), _full((D,)), _full((D,))
    _raw_losses_bnres(src, e, idx, dz_scale, dz_add, loss, dz, dg, db)          # 256 < D <= 1024: the entry point's own range
    return loss, dz, dg, db


def _check_losses(ref, loss, dz, what):
    bf16 = dz.dtype == BF16
    assert abs(loss.item() - ref.loss) <= 1e-6 * abs(ref.loss), f"{what}: loss {loss.item()!r} vs {ref.loss!r}"
    _note("losses", abs(loss.item() - ref.loss) / (1e-6 * abs(ref.loss)), what)
    _within("loss gradients" + (" (bf16)" if bf16 else " (fp32)"), dz, ref.dz, R.dz_bound(ref, bf16), what + " dz")


def _check_bn_sums(dz, x, mean, invstd, dg, db, what):
    w_dg, w_db, t_dg, t_db = R.bn_sums_ref(dz, x, mean, invstd)          # of dz AS STORED
    _within("BatchNorm sums of dz", dg, w_dg, R.BN_SUM_TOL * t_dg, what + " dgamma")
    _within("BatchNorm sums of dz", db, w_db, R.BN_SUM_TOL * t_db, what + " dbeta")


@pytest.mark.parametrize("N,D,why", R.LOSS_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_losses_indexed(N, D, why):
    """Plain, with bn=, and on sources (D <= 1024); fp32 and bf16 gradients, with and without dz_add; a few indices outside
    [0, K) give the result of the clamped index, bit for bit."""
    d = R.make_loss_inputs(N, D)
    K, scale = d.K, 0.25
    assert R.losses_chain(N, D) < 300
    zg, eg, idxg = gpu(d.z), gpu(d.e), gpu(d.idx)
    clamped = gpu(R.clamp_index(d.idx, K))
    meang, invstdg = gpu(d.mean), gpu(d.invstd)
    tag = f"losses ({N}, {D})"
    for dt in (F32, BF16):
        add = d.add.to(dt)
        xs = d.x.to(dt)
        addg, xg = gpu(add), gpu(xs)
        for with_add in (True, False):
            a, ag = (add, addg) if with_add else (None, None)
            what = f"{tag} {'bf16' if dt == BF16 else 'fp32'}{' +add' if with_add else ''}"

            def plain(ix):
                _poison((N, D), dt)
                return ops.vq_losses_indexed(zg, eg, ix, dz_scale=scale, dz_add=ag, grad_dtype=dt)

            def with_bn(ix):
                _poison((N, D), dt)
                return ops.vq_losses_indexed(zg, eg, ix, dz_scale=scale, dz_add=ag, grad_dtype=dt, bn=(xg, meang, invstdg),
                                             dgamma=_full((D,)), dbeta=_full((D,)))
            loss, dz = _twice(lambda: plain(idxg))
            lossc, dzc = plain(clamped)
            assert torch.equal(loss, lossc) and torch.equal(dz, dzc), f"{what}: a bad index is not the clamped index"
            loss_b, dz_b, dg, db = _twice(lambda: with_bn(idxg))
            for u, v in zip(with_bn(clamped), (loss_b, dz_b, dg, db)):
                assert torch.equal(u, v), f"{what}: bn form, a bad index is not the clamped index"
            # the existing relation: the bn form's loss and dz are the plain form's, bit for bit
            assert torch.equal(loss_b, loss) and torch.equal(dz_b, dz)
            # against fp64: everything below 2^20 elements; above, the loss and dz for (fp32, add) and (bf16, no add), the sums
            # of dz as stored for (fp32, no add) and (bf16, add) -- the fp64 passes over 8 M elements are what takes the time
            small = N * D <= (1 << 20)
            if small or (dt == F32) == with_add:
                _check_losses(R.losses_ref(d.z, d.e, d.idx, scale, a), loss, dz, what)
            if small or (dt == F32) != with_add:
                _check_bn_sums(dz_b, xs, d.mean, d.invstd, dg, db, what)
    if D > 1024:
        return
    src = _sources(d.src)
    zsg = gpu(d.z_src)
    for with_add in (True, False):
        add = d.add.to(BF16)
        a, ag = (add, gpu(add)) if with_add else (None, None)
        what = f"{tag} on sources{' +add' if with_add else ''}"
        loss, dz, dg, db = _twice(lambda: _losses_on_sources(src, eg, idxg, scale, ag))
        for u, v in zip(_losses_on_sources(src, eg, clamped, scale, ag), (loss, dz, dg, db)):
            assert torch.equal(u, v), f"{what}: a bad index is not the clamped index"
        _check_losses(R.losses_ref(d.z_src, d.e, d.idx, scale, a), loss, dz, what)
        _check_bn_sums(dz, d.src[0], d.src[2], d.src[3], dg, db, what)          # (h, mean, invstd)
        # the existing relation: bit for bit the bn form on the materialised rows (here: the rows formed on the CPU)
        l2, dz2, dg2, db2 = ops.vq_losses_indexed(zsg, eg, idxg, dz_scale=scale, dz_add=ag, grad_dtype=BF16, bn=(src.h, src.mean, src.invstd))
        assert torch.equal(l2, loss) and torch.equal(dz2, dz) and torch.equal(dg2, dg) and torch.equal(db2, db)


# ----------------------------------------------------------------------------------------------------------------------
# EMA update
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D", R.EMA_CASES, ids=str)
def test_ema_update(K, D):
    """(8192, 256) needs a second stride of the 2048-block grid; some codes have a running count and a batch count of 0."""
    d = R.make_ema_inputs(K, D)
    ref = R.ema_ref(d.ema_n, d.ema_s, d.n, d.s)
    ng, sg = gpu(d.n), gpu(d.s)

    def run():
        e, en, es = _full((K, D)), gpu(d.ema_n.clone()), gpu(d.ema_s.clone())          # the old codebook is not read: NaN shows a skipped element
        ops.vq_ema_update(e, en, es, ng, sg, decay=R.EMA_DECAY, eps=R.EMA_EPS)
        return e, en, es
    e, en, es = _twice(run)
    what = f"ema ({K}, {D})"
    _within("ema statistics", en, ref.ema_n, ref.b_n, what + " ema_n")
    _within("ema statistics", es, ref.ema_s, ref.b_s, what + " ema_s")
    _within("ema codebook", e, ref.e, ref.b_e, what + " codebook")
    if K > 1:
        assert not bool(en[gpu(d.dead)].any())


# ----------------------------------------------------------------------------------------------------------------------
# rejections launch nothing
# ----------------------------------------------------------------------------------------------------------------------
def _mis(t):
    """A contiguous copy of t that starts at element 1 of its buffer: not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _untouched(*ts):
    torch.cuda.synchronize()
    for t in ts:
        if t.dtype == I64:
            assert bool((t == R.IDX_POISON).all()), "a refused call wrote its index output"
        else:
            assert bool(torch.isnan(t.float()).all()), "a refused call wrote an output"


def test_search_rejections_launch_nothing():
    g = torch.Generator().manual_seed(1)
    N, K = 16, 8
    # D % 8 != 0 or D > 256 for bf16x3; D > 256 for the exact search
    for D in (12, 264, 257):
        x, e = gpu(torch.randn(N, D, generator=g)), gpu(torch.randn(K, D, generator=g))
        idx, codes, dmin, lp = _full((N,), I64), _full((N, D)), _full((N,)), _full((N, D), BF16)
        with pytest.raises(NsgError):
            _raw_bf16x3(x, e, idx, codes, dmin, lp, True, None, 0)
        with pytest.raises(NsgError):
            ops.vq_forward(x, e, impl="bf16x3")
        if D > 256:
            ws, nb = ops._ws(e.device, "nsg_vq_workspace_bytes", N, D, K)
            with pytest.raises(NsgError):
                _lib.call("nsg_vq_forward", ops._p(x), ops._p(e), N, D, K, ops._p(idx), ops._p(codes), ops._p(dmin), ops._p(ws), nb, ops._stream())
            with pytest.raises(NsgError):
                ops.vq_forward(x, e)
            if D % 8 == 0:
                src = ops.BnResRows(x.to(BF16), x.to(BF16), *[torch.ones(D, device=DEV)] * 4)
                with pytest.raises(NsgError):
                    _raw_bf16x3_bnres(src, e, idx, lp, True, None, 0)
        _untouched(idx, codes, dmin, lp)
    # misaligned views: every pointer the bf16x3 entry points want 16-byte aligned
    D = 16
    x, e, rows = gpu(torch.randn(N, D, generator=g)), gpu(torch.randn(K, D, generator=g)), gpu(torch.randn(2, D, generator=g))
    idx, codes, dmin, lp = _full((N,), I64), _full((N, D)), _full((N,)), _full((N, D), BF16)
    for args in ((_mis(x), e, idx, codes, dmin, lp, False, None, 0), (x, _mis(e), idx, codes, dmin, lp, False, None, 0),
                 (x, e, idx, _mis(codes), dmin, lp, False, None, 0), (x, e, idx, codes, dmin, _mis(lp), False, None, 0),
                 (x, e, idx, codes, dmin, lp, False, _mis(rows), N // 2)):
        with pytest.raises(NsgError):
            _raw_bf16x3(*args)
    with pytest.raises(NsgError):
        ops.vq_forward(_mis(x), e, impl="bf16x3")
    src = ops.BnResRows(x.to(BF16), x.to(BF16), *[torch.ones(D, device=DEV)] * 4)
    for bad in (src._replace(h=_mis(src.h)), src._replace(r=_mis(src.r))):
        with pytest.raises(NsgError):
            _raw_bf16x3_bnres(bad, e, idx, lp, True, None, 0)
        with pytest.raises(NsgError):
            ops.vq_forward(bad, e, want_codes=False, impl="bf16x3", codes_bf16="relu")
    # clip_rows without codes_bf16: the library refuses it; the wrapper does before it gets there
    with pytest.raises(NsgError):
        _raw_bf16x3(x, e, idx, codes, dmin, None, False, rows, N // 2)
    with pytest.raises((NsgError, ValueError)):
        ops.vq_forward(x, e, impl="bf16x3", clip_rows=rows)
    # sources passed to forms that do not take them
    with pytest.raises(NsgError):
        ops.vq_forward(src, e)                                                          # the exact search
    with pytest.raises(NsgError):
        ops.vq_forward(src, e, want_codes=False, want_dist=True, impl="bf16x3")        # distances need the rows
    with pytest.raises(NsgError):
        ops.vq_forward(src, e, want_codes=True, impl="bf16x3")                         # fp32 codes
    _untouched(idx, codes, dmin, lp)


def test_index_add_rejections_launch_nothing():
    g = torch.Generator().manual_seed(2)
    N, D = 64, 16

    def sorted_raw(idx, rows, K, out, counts):
        ws, nb = ops._ws(out.device, "nsg_index_add_sorted_workspace_bytes", N, rows.shape[1], K)
        _lib.call("nsg_index_add_rows_sorted", ops._p(idx), ops._p(rows), N, rows.shape[1], K, ops._p(out), ops._p(counts), ops._p(ws), nb, ops._stream())
    rows, idx = gpu(torch.randn(N, D, generator=g)), gpu(torch.randint(0, 8, (N,), generator=g))
    # K > 8192
    out, counts = _full((8193, D)), _full((8193,))
    assert not ops.index_add_sorted_supported(N, D, 8193)
    with pytest.raises(NsgError):
        sorted_raw(idx, rows, 8193, out, counts)
    _untouched(out, counts)
    # misaligned rows / out, in every form
    K = 8
    out, counts = _full((K, D)), _full((K,))
    with pytest.raises(NsgError):
        sorted_raw(idx, _mis(rows), K, out, counts)
    with pytest.raises(NsgError):
        sorted_raw(idx, rows, K, _mis(out), counts)
    for impl in ("sorted", "f32", "bf16x2"):
        with pytest.raises(NsgError):
            ops.index_add_rows(idx, _mis(rows), K, impl=impl, out=out)
    wide = gpu(torch.randn(N, 64, generator=g))          # (bf16x2 runs the bf16 pipe from D = 40 on)
    out64 = _full((K, 64))
    with pytest.raises(NsgError):
        ops.index_add_rows(idx, _mis(wide), K, impl="bf16x2", out=out64)
    src = ops.BnResRows(rows.to(BF16), rows.to(BF16), *[torch.ones(D, device=DEV)] * 4)
    for bad in (src._replace(h=_mis(src.h)), src._replace(r=_mis(src.r))):
        with pytest.raises(NsgError):
            ops.index_add_rows(idx, bad, K, impl="sorted", out=out, counts=counts)
    with pytest.raises(NsgError):
        _raw_sorted_bnres(idx, src, K, _mis(out), counts)
    # sources passed to the one-hot forms; a width the _bnres form does not take
    for impl in ("f32", "bf16x2"):
        with pytest.raises(NsgError):
            ops.index_add_rows(idx, src, K, impl=impl, out=out)
    src24 = ops.BnResRows(torch.zeros(N, 24, dtype=BF16, device=DEV), torch.zeros(N, 24, dtype=BF16, device=DEV), *[torch.ones(24, device=DEV)] * 4)
    out24 = _full((K, 24))
    with pytest.raises(NsgError):
        _raw_sorted_bnres(idx, src24, K, out24, None)
    _untouched(out, counts, out64, out24)


def test_losses_rejections_launch_nothing():
    g = torch.Generator().manual_seed(3)
    N, D, K = 16, 16, 8
    z, e, idx = gpu(torch.randn(N, D, generator=g)), gpu(torch.randn(K, D, generator=g)), gpu(torch.randint(0, K, (N,), generator=g))
    mean, invstd = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    for dt in (F32, BF16):
        add, x = torch.zeros(N, D, dtype=dt, device=DEV), torch.zeros(N, D, dtype=dt, device=DEV)
        for kw in (dict(z=_mis(z)), dict(e=_mis(e)), dict(add=_mis(add)), dict(x=_mis(x))):
            a = dict(z=z, e=e, add=add, x=x)
            a.update(kw)
            if "x" not in kw:
                with pytest.raises(NsgError):
                    ops.vq_losses_indexed(a["z"], a["e"], idx, dz_add=a["add"], grad_dtype=dt)
            with pytest.raises(NsgError):
                ops.vq_losses_indexed(a["z"], a["e"], idx, dz_add=a["add"], grad_dtype=dt, bn=(a["x"], mean, invstd))
    # a misaligned dz: the entry points themselves, on poisoned outputs
    loss, dz, dg, db = _full((1,)), _full((N, D), BF16), _full((D,)), _full((D,))
    ws, nb = ops._ws(e.device, "nsg_vq_losses_indexed_bn_workspace_bytes", N, D)
    with pytest.raises(NsgError):
        _lib.call("nsg_vq_losses_indexed", ops._p(z), ops._p(e), ops._p(idx), N, D, K, 1.0, ops._p(None), ops._p(loss), ops._p(_mis(dz)), ops.nsg_dtype(BF16),
                  ops._p(ws), nb, ops._stream())
    src = ops.BnResRows(z.to(BF16), z.to(BF16), mean, invstd, torch.ones(D, device=DEV), torch.zeros(D, device=DEV))
    add = torch.zeros(N, D, dtype=BF16, device=DEV)
    for bad_src, bad_e, bad_add, bad_dz in ((src._replace(h=_mis(src.h)), e, add, dz), (src._replace(r=_mis(src.r)), e, add, dz), (src, _mis(e), add, dz),
                                            (src, e, _mis(add), dz), (src, e, add, _mis(dz))):
        with pytest.raises(NsgError):
            _raw_losses_bnres(bad_src, bad_e, idx, 1.0, bad_add, loss, bad_dz, dg, db)
    # widths: D % 8 != 0; above 2048 (_bn) and above 1024 (_bnres)
    for D2, bnres_only in ((12, False), (2056, False), (1032, True)):
        z2, e2 = torch.zeros(N, D2, device=DEV), torch.zeros(K, D2, device=DEV)
        v = torch.ones(D2, device=DEV)
        loss2, dz2, dg2, db2 = _full((1,)), _full((N, D2), BF16), _full((D2,)), _full((D2,))
        if not bnres_only:
            with pytest.raises(NsgError):
                ops.vq_losses_indexed(z2, e2, idx, grad_dtype=BF16)
            with pytest.raises(NsgError):
                ops.vq_losses_indexed(z2, e2, idx, grad_dtype=BF16, bn=(z2.to(BF16), v, v))
        if D2 % 8 == 0:
            s2 = ops.BnResRows(z2.to(BF16), z2.to(BF16), v, v, v, v)
            with pytest.raises(NsgError):
                _raw_losses_bnres(s2, e2, idx, 1.0, None, loss2, dz2, dg2, db2)
            _untouched(loss2, dz2, dg2, db2)
    # sources passed to forms that do not take them
    with pytest.raises(NsgError):
        ops.vq_losses_indexed(src, e, idx, grad_dtype=BF16)                                            # without bn=
    with pytest.raises(NsgError):
        ops.vq_losses_indexed(src, e, idx, grad_dtype=F32, bn=(src.h, src.mean, src.invstd))          # fp32 gradients
    with pytest.raises(NsgError):
        ops.vq_losses_indexed(src, e, idx, grad_dtype=BF16, bn=(src.r, src.mean, src.invstd))         # another BatchNorm's input
    _untouched(loss, dz, dg, db)


def test_report_largest_errors():
    """Not a check: the largest error / bound each tolerance class met in this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[vq envelope] {cls}: largest error / bound = {WORST[cls][0]:.4f} at {WORST[cls][1]}")
