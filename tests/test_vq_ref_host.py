"""The quantiser's fp64 yardstick (tests/helpers/vq_ref64.py) checked on the CPU: that it is RIGHT -- a CPU emulation of the
split search (hi / lo split, three products, fp32 accumulation) stays inside the derived bound on every search case, the integer
probes meet their exactness preconditions, the chain lengths are the ones the case tables claim, the restated shape rules are
the library's -- and that it is SHARP: every acceptance rule is fed deliberately wrong results, the ones a subtly broken kernel
would produce, and must reject each.  That is the evidence that tests/test_gpu_vq_envelope.py fails on such a kernel; no broken
kernel is built for it."""
import numpy as np
import pytest
import torch

from neural_sound_generation_amd import ops
from tests.helpers import bn_ref64
from tests.helpers import vq_ref64 as R

WORST = {}


def _note(cls, v, where):
    if v > WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (v, where)


@pytest.fixture(scope="module", params=R.SEARCH_CASES, ids=R.search_case_id)
def scase(request):
    N, K, D, data = request.param
    c = R.make_search_inputs(N, K, D, data)
    c.tag = R.search_case_id(request.param)
    c.ops = {"x": (c.x, c.e_x, c.planted_x, R.search_ref(c.x, c.e_x)), "z": (c.z, c.e_z, c.planted_z, R.search_ref(c.z, c.e_z))}
    return c


# ----------------------------------------------------------------------------------------------------------------------
# the search: the bound holds for an honest split search ...
# ----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_envelope():
    cases = R.SEARCH_CASES
    assert {c[0] for c in cases} == set(R.SEARCH_N) and {c[1] for c in cases} == set(R.SEARCH_K) | {8192}
    assert sum(1 for c in cases if c[1] == 8192) == 1
    for D in R.SEARCH_D:
        mine = [c for c in cases if c[2] == D]
        assert {c[3] for c in mine} == set(R.SEARCH_DATA), f"D = {D} misses a kind of data"
        assert len({c[0] for c in mine}) >= 3 and len({c[1] for c in mine}) >= 3
    assert {(c[0], c[1]) for c in cases} >= {(n, k) for n in R.SEARCH_N for k in R.SEARCH_K}
    # every padded width with D < DP and with D = DP
    for dp in (16, 32, 64, 128, 256):
        ds = [c[2] for c in cases if R.dp_of(c[2]) == dp]
        assert dp in ds and any(D < dp for D in ds)
    assert {R.dp_of(D) for D in (136, 248)} == {256}
    assert R.SEARCH_ROWS_LEFT_OUT == 0


def test_split_emulation_stays_inside_the_bound(scase):
    c = scase
    for name, (x, e, planted, ref) in c.ops.items():
        # the planted codes are what they are meant to be: the unique first minimum of their rows
        for what, (row, code) in planted.items():
            assert int(ref.argmin[row]) == code, f"{c.tag} {name}: planted '{what}' is not the first minimum of row {row}"
        for has_x2 in (False, True):
            d, idx = R.emulate_split_search(x, e, has_x2)
            true = ref.dist if has_x2 else ref.dist - (R.f64(x) ** 2).sum(1)[:, None]
            bound = ref.bound_dmin if has_x2 else ref.bound_plain
            ratio = float(((d.double() - true).abs() / bound).max())
            _note("emulated distance error / bound", ratio, f"{c.tag} {name} x2={has_x2}")
            assert ratio <= 1.0, f"{c.tag} {name} x2={has_x2}: the emulation leaves the bound ({ratio:.3f})"
            dmin = d.min(1).values if has_x2 else None
            bad = R.search_violations(ref, idx, dmin)
            assert int(bad.sum()) == R.SEARCH_ROWS_LEFT_OUT, f"{c.tag} {name}: the rule rejects {int(bad.sum())} rows of an honest search"
            if c.data == "int":
                assert not bool(R.int_violations(x, e, idx, dmin).any()), f"{c.tag} {name}: the emulation is not exact on integers"
        if c.data == "gauss" and c.K > 1:
            # how sharp: the gap to the second-nearest code against the slack (reported, not asserted)
            two = ref.dist.topk(2, dim=1, largest=False)
            slack = ref.bound_plain.gather(1, two.indices).sum(1)
            gap = two.values[:, 1] - two.values[:, 0]
            _note("median gap / slack (smallest case)", -float((gap / slack).median()), f"{c.tag} {name}")


def test_integer_probe_preconditions(scase):
    c = scase
    if c.data != "int":
        assert bool((c.x != c.x.round()).any())          # (the other kinds are no integer probes: nothing to establish)
        return
    for x, e, planted, _ in c.ops.values():
        idx, dmin = R.int_exact(x, e)          # asserts integer entries, D * max|v|^2 < 2^23, integer distances below 2^24
        hi, lo = R.split_bf16(x)
        assert torch.equal(hi, x) and not bool(lo.any())          # the split is exact: the three forms see the integers
        assert float(x.abs().max()) <= 3 and float(e.abs().max()) <= 3
        d = (R.f64(x) ** 2).sum(1)[:, None] + (R.f64(e) ** 2).sum(1)[None, :] - 2.0 * R.f64(x) @ R.f64(e).t()
        ties = int(((d == d.min(1, keepdim=True).values).sum(1) > 1).sum())
        if c.N >= 3 and c.K >= 8:
            assert ties >= 1, "no tie at a minimum: the probe pins no tie rule"
    # the sources reproduce integers exactly
    assert bool((c.z == c.z.round()).all()) and float(c.z.abs().max()) <= 3


# ... and the rule rejects what a broken kernel would return
def test_search_rule_rejects_wrong_results(scase):
    c = scase
    for name, (x, e, planted, ref) in c.ops.items():
        x64, e64 = R.f64(x), R.f64(e)
        x2, e2 = (x64 * x64).sum(1), (e64 * e64).sum(1)
        honest = ref.argmin.clone()
        tag = f"{c.tag} {name}"

        def rejected(idx, dmin_of=None):
            """Both forms: the production form judges the index alone, the dmin form the index and the distance."""
            plain = bool(R.search_violations(ref, idx).any())
            dm = ref.dist.gather(1, idx.clamp(0, c.K - 1)[:, None])[:, 0].float() if dmin_of is None else dmin_of
            return plain, bool(R.search_violations(ref, idx, dm).any())

        assert rejected(honest) == (False, False)
        # the last code tile ignored
        if c.K > 32:
            kk = 32 * ((c.K - 1) // 32)
            idx = R.first_argmin(ref.dist[:, :kk])
            assert rejected(idx) == (True, True), f"{tag}: a search that ignores the last code tile passes"
        # channels at and beyond the last full 16 ignored in the dot product (the norms are whole)
        if "tail" in planted:
            t0 = R.tail_start(c.D)
            d = x2[:, None] + e2[None, :] - 2.0 * (x64[:, :t0] @ e64[:, :t0].t())
            idx = R.first_argmin(d)
            assert int(idx[planted["tail"][0]]) != planted["tail"][1]
            assert rejected(idx, d.min(1).values.float()) == (True, True), f"{tag}: a search that ignores channels {t0}.. passes"
        # the last 128-row block left unwritten (poisoned outputs)
        idx = honest.clone()
        idx[128 * ((c.N - 1) // 128):] = R.IDX_POISON
        dm = ref.dmin.float().clone()
        dm[128 * ((c.N - 1) // 128):] = float("nan")
        assert rejected(idx, dm) == (True, True), f"{tag}: an unwritten last block passes"
        assert bool(R.search_violations(ref, honest, dm).any()), f"{tag}: an unwritten dmin passes"
        # a wrong reported distance: the neighbouring code's
        if c.K > 1:
            other = ref.dist.gather(1, ((honest + 1) % c.K)[:, None])[:, 0].float()
            assert bool(R.search_violations(ref, honest, other).any()), f"{tag}: another code's distance passes as dmin"
        # ties resolved to the LAST index: only the integer probe pins the rule (equal distances are equally near)
        if c.data == "int":
            d = x2[:, None] + e2[None, :] - 2.0 * (x64 @ e64.t())
            last = R.last_argmin(d)
            if not torch.equal(last, honest):
                assert bool(R.int_violations(x, e, last).any()), f"{tag}: ties resolved to the last index pass the integer probe"
            assert "dup_tile" not in planted or int(last[planted["dup_tile"][0]]) == 5
            assert not bool(R.int_violations(x, e, honest, ref.dmin.float()).any())
            assert bool(R.int_violations(x, e, honest, ref.dmin.float() + 1.0).any())


@pytest.mark.parametrize("rpc,clips", R.CLIP_CASES, ids=str)
def test_code_output_rule_rejects_wrong_results(rpc, clips):
    """codes_bf16 is compared bit for bit: the neighbouring clip's row and a dropped ReLU change bits."""
    N, D, K = rpc * clips, 16, 20
    g = torch.Generator().manual_seed(rpc)
    e, rows = torch.randn(K, D, generator=g), torch.randn(clips, D, generator=g) * 0.3
    idx = torch.randint(0, K, (N,), generator=g)
    for relu in (False, True):
        want = R.codes_bf16_ref(e, idx, rows, rpc, relu)
        assert want.dtype == torch.bfloat16 and want.shape == (N, D)
        wrong = R.codes_bf16_ref(e, idx, rows, rpc, relu, clip_shift=1)
        assert not torch.equal(wrong, want)
        # a boundary off by one row: row rpc takes clip 0's row
        off = want.clone()
        off[rpc] = R.codes_bf16_ref(e, idx, rows, rpc, relu, clip_shift=-1)[rpc]
        assert not torch.equal(off, want)
        assert not torch.equal(R.codes_bf16_ref(e, idx, None, 0, relu), want)          # the clip row not added at all
    assert not torch.equal(R.codes_bf16_ref(e, idx, rows, rpc, False), R.codes_bf16_ref(e, idx, rows, rpc, True))       # ReLU dropped
    assert float(R.codes_bf16_ref(e, idx, rows, rpc, True).float().min()) == 0.0
    # the 128-row blocks of the three cases: three clips in one block / one clip / a boundary one row into the second block
    assert (rpc, len({r // rpc for r in range(min(N, 128))})) in ((50, 3), (128, 1), (129, 1))


def test_exact_search_cases_reach_their_slices():
    for N, D, K, S, _ in R.EXACT_CASES:
        assert R.vq_slices(N, D, K) == S, (N, D, K)
        x, e, must = R.make_exact_inputs(N, D, K, S)
        per = 32 * R.slice_tiles(K, S)
        assert (S - 1) * per < K <= S * per
        if S > 1:
            assert len(must) >= 2
        for row, a in must.items():
            twins = [k for k in range(K) if np.array_equal(e[k], x[row])]
            assert twins[0] == a and len(twins) == 2 and twins[0] // per != twins[1] // per, "the duplicates share a slice"
    assert {c[3] for c in R.EXACT_CASES} == {1, 2, 4, 8}
    assert any(K % (32 * S) for _, _, K, S, _ in R.EXACT_CASES if S == 8)
    # the slice rule itself at the shapes the library's tests already pin (test_vq_full_size_properties: S = 4 and 8)
    assert R.vq_slices(81920, 256, 8192) in (1, 2, 4, 8) and R.vq_slices(1, 128, 512) == 1


# ----------------------------------------------------------------------------------------------------------------------
# segment sums
# ----------------------------------------------------------------------------------------------------------------------
def test_segment_case_table_and_chains():
    cases = R.SEG_CASES
    small = [c for c in cases if c[0] <= 1025]
    assert {c[0] for c in small} == set(R.SEG_N) and {c[1] for c in cases} == set(R.SEG_K) and {c[2] for c in cases} == set(R.SEG_D)
    for n in R.SEG_N:
        assert len({c[2] for c in small if c[0] == n}) >= 4 and {c[4] for c in small if c[0] == n} == {"gauss", "int"}
    assert {c[3] for c in cases} == {"uniform", "skew", "oob_mixed", "collapsed", "oob_all"}
    for c in cases:
        assert R.sorted_supported(c[0], c[2], c[1])
    # the multi-pass scan: more than 8 * 96 blocks of 1024 rows
    assert -(-R.SEG_BIG_N // R.SEG_ROWS) == 770 > R.SEG_SCAN_PASS and R.SEG_BIG_N == 786432 + 1025
    assert sum(1 for c in cases if c[0] == R.SEG_BIG_N) >= 2
    # chains, by hand: D = 256 (one row per load, 4 groups), 1000 rows: 128 + 0 + 4 + ceil(2 / 4) + 4
    assert int(R.sorted_chain(np.array([1000]), 256)[0]) == 128 + 0 + 4 + 1 + 4
    # D = 512 (wide rows, one group): 512 rows of the first chunk, then 2 chunks + 1
    assert int(R.sorted_chain(np.array([1000]), 512)[0]) == 512 + 2 + 1
    # D = 16: 4 pieces, 16 rows per load, 64 groups; 130 rows: ceil(128 / 16) + 15 + 4 + 1 + 64
    assert int(R.sorted_chain(np.array([130]), 16)[0]) == 8 + 15 + 4 + 1 + 64
    for key, (form, want) in R.SEG_CHAIN_CLAIMS.items():
        c = next(c for c in cases if c[:4] == key)
        d = R.make_seg_inputs(*c)
        ref = R.seg_ref(d.idx, d.g, d.K)
        assert int(R.sorted_chain(ref.counts.numpy(), d.D).max()) == want, key
    # the one-hot plan at the big case: 512 slabs wanted, 1568 rows each (a multiple of 32), 503 slabs
    assert R.onehot_plan(R.SEG_BIG_N, 7, 4) == (503, 1568)
    assert R.onehot_plan(1, 1, 4) == (1, 32) and R.onehot_plan(1025, 8192, 512) == (2, 544)          # 256 tiles: two slabs of ceil(513 / 32) * 32 rows
    assert int(R.onehot_chain(np.array([5000]), R.SEG_BIG_N, 7, 4, False)[0]) == 1568 + 503 + 1
    assert int(R.onehot_chain(np.array([10]), 1025, 7, 64, True)[0]) == 20 + R.onehot_plan(1025, 7, 64)[0] + 1


def test_sorted_shape_rule_is_the_librarys():
    """One rule in three places: this helper, ops.index_add_sorted_supported (and include/nsg.h, which the C check follows)."""
    for D in range(1, 1300):
        for N, K in ((1, 1), (1000, 8192), (5, 8193)):
            assert R.sorted_supported(N, D, K) == bool(ops.index_add_sorted_supported(N, D, K)), (N, D, K)
    assert not R.sorted_supported(64, 260, 8) and R.sorted_supported(64, 256, 8) and R.sorted_supported(64, 768, 8)
    assert not R.sorted_supported(64, 12, 8) and not R.sorted_supported(64, 384, 8)
    assert [D for D in range(1, 300) if R.bnres_sorted_supported(D)] == [4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("case", R.SEG_CASES, ids=R.seg_case_id)
def test_segment_rule_rejects_wrong_results(case):
    d = R.make_seg_inputs(*case)
    ref = R.seg_ref(d.idx, d.g, d.K)
    exact = d.data == "int"
    valid = ((d.idx >= 0) & (d.idx < d.K)).nonzero()[:, 0]
    assert int(ref.counts.sum()) == valid.numel()
    if d.kind == "oob_all":
        assert valid.numel() == 0 and not bool(ref.sums.any())
    honest, hcounts = ref.sums.float(), ref.counts.float()
    for impl in ("sorted", "f32", "bf16x2"):
        assert R.seg_violations(impl, ref, honest, hcounts, exact) == 0
        nan = honest.clone()
        nan[d.K - 1, d.D - 1] = float("nan")          # an element never written
        assert R.seg_violations(impl, ref, nan, hcounts, exact) > 0
    if exact:
        assert float(ref.absum.max()) < 2 ** 24
    detectable = exact or d.N <= 1025          # a Gaussian row of 787 457 hides inside the chain bound: the integer data catches it
    for row in ([int(valid[0]), int(valid[-1])] if valid.numel() else []):
        k = int(d.idx[row])
        for sign, what in ((-1.0, "lost"), (1.0, "counted twice")):
            wrong, wc = honest.double().clone(), hcounts.clone()
            wrong[k] += sign * d.g[row].double()
            wc[k] += sign
            assert R.seg_violations("sorted", ref, honest, wc, exact) > 0, f"row {row} {what}: the counts pass"
            if detectable and bool(d.g[row].any()):
                for impl in ("sorted", "f32", "bf16x2"):
                    assert R.seg_violations(impl, ref, wrong.float(), None, exact) > 0, f"row {row} {what}: the {impl} sums pass"
    # an index taken modulo 2^32: 2^32 + 3 joins code 3, -2^32 + 1 code 1, 2^32 code 0
    if d.kind in ("oob_mixed", "oob_all"):
        low = d.idx & 0xFFFFFFFF
        low = torch.where(low >= 2 ** 31, low - 2 ** 32, low)
        mod = R.seg_ref(low, d.g, d.K)
        lands = int(mod.counts.sum()) > int(ref.counts.sum())
        assert lands or d.N < len(R.BAD_INDICES), "no bad index lands in range modulo 2^32"
        assert not lands or R.seg_violations("sorted", ref, honest, mod.counts.float(), exact) > 0
        if detectable and lands:
            for impl in ("f32", "bf16x2"):
                assert R.seg_violations(impl, ref, mod.sums.float(), None, exact) > 0, f"sums with indices modulo 2^32 pass ({impl})"


# ----------------------------------------------------------------------------------------------------------------------
# losses, EMA
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,_", R.LOSS_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_losses_rule_rejects_wrong_results(N, D, _):
    assert R.losses_chain(N, D) < bn_ref64.MAX_CHAIN
    assert bn_ref64.MAX_CHAIN * R.U32 < R.BN_SUM_TOL
    if N * D > (1 << 21):
        N = 4097          # the rule is the same; the host test does not need the largest tensors twice
    d = R.make_loss_inputs(N, D)
    assert int(((d.idx < 0) | (d.idx >= d.K)).sum()) >= 1
    for bf16, add in ((False, d.add), (True, d.add.bfloat16()), (True, None)):
        ref = R.losses_ref(d.z, d.e, d.idx, 0.25, add)
        honest = ref.dz.bfloat16() if bf16 else ref.dz.float()
        assert R.losses_violations(ref, np.float32(ref.loss), honest, bf16) == 0
        # a clamp missing: the bad index wraps instead
        wrong = R.losses_ref(d.z, d.e, d.idx, 0.25, add, clamp=False)
        wdz = wrong.dz.bfloat16() if bf16 else wrong.dz.float()
        assert R.losses_violations(ref, np.float32(ref.loss), wdz, bf16) > 0, "dz of a wrapped index passes"
        if N <= 65:
            assert R.losses_violations(ref, np.float32(wrong.loss), honest, bf16) > 0, "the loss of a wrapped index passes"
        # the last row unwritten
        nan = honest.clone()
        nan[-1] = float("nan")
        assert R.losses_violations(ref, np.float32(ref.loss), nan, bf16) > 0
        # the BatchNorm sums are those of dz AS STORED: one row dropped from them is outside the bound
        dg, db, tg, tb = R.bn_sums_ref(honest, d.x, d.mean, d.invstd)
        dg2, db2, _, _ = R.bn_sums_ref(honest[:-1], d.x[:-1], d.mean, d.invstd)
        if 1 < N <= 4097:          # (one Gaussian row of 65 601 is inside 2e-5 of the column)
            assert bool(((db2 - db).abs() > R.BN_SUM_TOL * tb).any())
    # the rows from their sources: fp32, formed in the header's order
    assert d.z_src.dtype == torch.float32 and d.z_src.shape == (N, D)
    h, r, mean, invstd, gam, beta = d.src
    z64 = (h.double() - mean.double()) * (invstd.double() * gam.double()) + beta.double() + r.double()
    assert float((d.z_src.double() - z64).abs().max()) <= 4 * R.U32 * float(z64.abs().max() + 3.0)


def test_bnres_rows_order_of_operations():
    """((h - mean) * (invstd * gamma) + beta) + r, one rounding each: bit for bit the expression written out in numpy fp32."""
    g = torch.Generator().manual_seed(5)
    src = R.make_sources(37, 24, "gauss", g)
    h, r, mean, invstd, gam, beta = (v.float().numpy() for v in src)
    want = ((h - mean) * (invstd * gam) + beta) + r
    assert want.dtype == np.float32 and np.array_equal(R.bnres_rows(*src).numpy(), want)
    other = (h - mean) * invstd * gam + (beta + r)          # another order rounds differently somewhere
    assert not np.array_equal(other, want)
    z = R.bnres_rows(*R.make_sources(5, 8, "int", g))
    assert bool((z == z.round()).all())


@pytest.mark.parametrize("K,D", R.EMA_CASES, ids=str)
def test_ema_reference(K, D):
    d = R.make_ema_inputs(K, D)
    ref = R.ema_ref(d.ema_n, d.ema_s, d.n, d.s)
    assert bool(torch.isfinite(ref.e).all()) and bool((ref.b_e >= 0).all())
    if K > 1:
        assert int(d.dead.sum()) >= 1 and not bool(ref.ema_n[d.dead].any())
        assert bool(ref.e[1].abs().max() > 1e3)          # a non-zero running sum over the tiny denominator of a dead code
        others = d.dead.clone()
        others[1] = False
        assert not bool(ref.e[others].any())
    # the formula, written out once more for one element
    k = K - 1
    dec, om = float(np.float32(0.99)), float(np.float32(1.0) - np.float32(0.99))
    vn = dec * d.ema_n.double() + om * d.n.double()
    nn = (vn[k] + float(np.float32(1e-5))) / (vn.sum() + K * float(np.float32(1e-5))) * vn.sum()
    want = (dec * float(d.ema_s[k, 0]) + om * float(d.s[k, 0])) / float(nn)
    assert abs(float(ref.e[k, 0]) - want) <= 1e-12 * max(1.0, abs(want))
    # an fp32 evaluation of the same formula stays inside the bounds; the old codebook left in place does not
    f = torch.float32
    vn32 = torch.tensor(0.99, dtype=f) * d.ema_n + (1 - torch.tensor(0.99, dtype=f)) * d.n
    vs32 = torch.tensor(0.99, dtype=f) * d.ema_s + (1 - torch.tensor(0.99, dtype=f)) * d.s
    tot32 = vn32.double().sum().float()
    e32 = vs32 / ((vn32 + 1e-5) / (tot32 + K * torch.tensor(1e-5, dtype=f)) * tot32)[:, None]
    assert bool(((e32.double() - ref.e).abs() <= ref.b_e).all())
    assert bool(((vn32.double() - ref.ema_n).abs() <= ref.b_n).all()) and bool(((vs32.double() - ref.ema_s).abs() <= ref.b_s).all())
    assert not bool(((d.e.double() - ref.e).abs() <= ref.b_e).all())
    assert 256 * 2048 < 8192 * 256          # the largest case needs a second stride of the 2048-block grid


def test_report():
    """Not a check: the figures of this module's run (shown with pytest -s)."""
    for cls in sorted(WORST):
        print(f"[vq yardstick] {cls}: {abs(WORST[cls][0]):.4f} at {WORST[cls][1]}")
