"""CPU: what tests/test_gpu_f0_cond_envelope.py relies on, checked without a device -- its launch constants against the sources
they are read from, its "second trip" shapes against the launch arithmetic, the rounding probes' exactness and the integer
rounding rule against torch, the order-sensitivity of the column-sum data, and the F0 cases against include/nsg.h's rule in fp64
and in fp32 (tests/helpers/f0_cond_envelope.py, f0_cond_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import test_gpu_f0_cond_envelope as G
from tests.helpers import f0_cond_envelope as E
from tests.helpers import f0_cond_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_sound_generation_amd", "csrc")
F32, BF16 = torch.float32, torch.bfloat16


def _body(text, start):
    """The text from `start` to the next line that closes a function at column 0."""
    at = text.index(start)
    return text[at:text.index("\n}", at)]


def test_launch_constants_are_the_sources():
    common = open(os.path.join(CSRC, "nsg_common.h")).read()
    ew = _body(common, "static inline int ew_blocks(int64_t n)")
    assert re.search(r"nsg_cdiv\(n, (\d+)\)", ew).group(1) == str(G.THREADS)
    assert re.search(r"b > (\d+) \? (\d+)", ew).groups() == (str(G.GRID_CAP),) * 2
    text = open(os.path.join(CSRC, "f0_cond.hip")).read()
    add_cond, column_sum = _body(text, "void add_cond_kernel("), _body(text, "void column_sum_kernel(")
    assert re.search(r"constexpr int U = (\d+);", add_cond).group(1) == str(G.ADD_COND_ITEMS)
    assert re.search(r"constexpr int U = (\d+);", column_sum).group(1) == str(G.COLUMN_SUM_ROWS)
    assert f"ew_blocks((nw + 1) / {G.ADD_COND_ITEMS})" in text and "ew_blocks(nv)" in text
    assert text.count("__launch_bounds__(%d)" % G.THREADS) == 4 and text.count(f"dim3({G.F0_BLOCK})") >= 2
    assert len(re.findall(r"nsg_cdiv\(\(int64_t\)B \* \w+, %d\)" % G.F0_BLOCK, text)) == 2


def test_second_trip_shapes_follow_from_the_constants():
    grid = G.GRID_CAP * G.THREADS
    for dtype in (F32, BF16):
        B, H, W, C = G.multi_trip_shape(dtype)
        nw = G.add_cond_vectors(B, H, W, C, dtype)
        assert (B, H, W, C) == (3, 5, 4370, G.MULTI_C[dtype]) and G.ADD_COND_ITEMS * grid < nw < G.ADD_COND_ITEMS * grid + B * H * (C // E.vec(dtype)) + 1
        assert G.add_cond_vectors(B, H, W - 1, C, dtype) <= G.ADD_COND_ITEMS * grid                 # the smallest such W
        blocks, trips, (whole, some, idle) = E.add_cond_launch(nw, G.GRID_CAP, G.THREADS, G.ADD_COND_ITEMS)
        assert (blocks, trips) == (G.GRID_CAP, 2) and (whole, some, idle) == (0, nw - 2 * grid, 3 * grid - nw)
        assert B * H * W * C <= 17_000_000                                                       # the CPU reference's size
        B, H, W, C = G.whole_items_shape(dtype)
        nw = G.add_cond_vectors(B, H, W, C, dtype)
        assert E.add_cond_launch(nw, G.GRID_CAP, G.THREADS, G.ADD_COND_ITEMS) == (G.GRID_CAP, 2, (nw - 3 * grid, 4 * grid - nw, 0)) and nw > 3 * grid
        assert B * H * W * C <= 26_000_000
        B, H, W, C = G.below_cap_shape(dtype)
        blocks, trips, (whole, some, idle) = E.add_cond_launch(G.add_cond_vectors(B, H, W, C, dtype), G.GRID_CAP, G.THREADS, G.ADD_COND_ITEMS)
        assert (blocks, trips) == (G.GRID_CAP - 1, 1) and whole > 0 and some > 0 and idle == 0
        B, H, W, C = G.column_sum_multi_trip_shape(dtype)
        assert (B, H, W, C) == ((2, 5, 4101, 512) if dtype == F32 else (4, 5, 4101, 512))
        nv = B * W * (C // E.vec(dtype))
        assert E.column_sum_launch(nv, G.GRID_CAP, G.THREADS) == (G.GRID_CAP, 2, nv - grid) and 0 < nv - grid < grid
        assert H // G.COLUMN_SUM_ROWS == 1 and H % G.COLUMN_SUM_ROWS == 1
        assert B * H * W * C * (2 if dtype == BF16 else 4) <= 84 * 2 ** 20
    assert G.column_sum_at_cap_shape() == (128, 2, 256, 128)
    # the launch arithmetic itself, at sizes small enough to count
    assert E.add_cond_launch(1, 4, 8, 2) == (1, 1, (0, 1, 7)) and E.add_cond_launch(16, 4, 8, 2) == (1, 1, (8, 0, 0))
    assert E.add_cond_launch(64, 4, 8, 2) == (4, 1, (32, 0, 0)) and E.add_cond_launch(65, 4, 8, 2) == (4, 2, (0, 1, 31))
    assert E.add_cond_launch(64 + 40, 4, 8, 2) == (4, 2, (8, 24, 0))
    assert E.column_sum_launch(33, 4, 8) == (4, 2, 1) and E.column_sum_launch(32, 4, 8) == (4, 1, 32)
    assert all(a % 16 == 0 for a in (G.GUARD16[F32] * 4, G.GUARD16[BF16] * 2))


def test_bf16_rule_is_torchs_rounding():
    rs = np.random.RandomState(0)
    pat = rs.randint(0, 2 ** 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    pat = pat[(pat & 0x7F800000) != 0x7F800000]                                             # finite
    t = E.rounding_probes()[0]
    for x in (pat.view(np.float32), t, np.maximum(t, np.float32(0))):
        want = torch.from_numpy(x.copy()).to(BF16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(E.bf16_bits_rne(x), want)
    # ... and the kinds are what their names say
    for kind, probes in E.ROUNDING_PROBES.items():
        p = np.array(probes, dtype=np.uint32)
        for sign in (0, 0x80000000):
            assert E.bf16_bits_rne((p | np.uint32(sign)).view(np.float32)).tolist() == [e | (sign >> 16) for e in E.ROUNDING_EXPECTED[kind]], kind
        low, kept = p & 0xFFFF, (p >> 16) & 1
        if kind.startswith("tie"):
            assert (low == 0x8000).all() and (kept == (1 if "odd" in kind else 0)).all()
        elif "below a tie" in kind:
            assert (low == 0x7FFF).all()
        elif "above a tie" in kind:
            assert (low == 0x8001).all()
        elif "subnormals" in kind:
            assert ((p >> 16) <= 0x7F).all() and {0x8000, 0x8001, 0x7FFF, 0x0000, 0x0001} == set(low.tolist())
    assert {int(k) for k in (np.array(E.ROUNDING_PROBES["tie, even lower neighbour"]) >> 16) & 1} == {0}


def test_rounding_probes_are_exact_sums():
    t, x, clip, table = E.rounding_probes()
    assert len(t) % 8 == 0 and np.isfinite(t).all() and t.dtype == x.dtype == clip.dtype == table.dtype == np.float32
    first = x.astype(np.float64) + clip.astype(np.float64)
    assert np.array_equal((x + clip).astype(np.float64), first)                             # fp32 rounds nothing away
    assert np.array_equal(((x + clip) + table).astype(np.float64), first + table.astype(np.float64))
    assert np.array_equal(((x + clip) + table).view(np.uint32), t.view(np.uint32))
    # torch's fp32 on the CPU agrees (no flush of subnormals): the reference the GPU test compares with
    tt = (torch.from_numpy(x.copy()) + torch.from_numpy(clip.copy())) + torch.from_numpy(table.copy())
    assert np.array_equal(tt.numpy().view(np.uint32), t.view(np.uint32))
    assert (t < 0).sum() == (t > 0).sum() - (t == 1.0).sum() and (table != 0).sum() > 0.8 * len(t)      # both signs; 1.0 pads


def test_clamp_values_tell_64_bits_from_32():
    for n in (5, 6):
        v = np.array(E.CLAMPED(n), dtype=np.int64)
        assert v.astype(np.int32).tolist() == E.TRUNCATED(n)
        full, low = np.clip(v, 0, n - 1), np.clip(v.astype(np.int32), 0, n - 1)
        assert full.tolist() == [0, n - 1, 0, n - 1, n - 1, n - 1, 0] and (full != low).sum() == 3
    d = E.add_cond_inputs(2, 3, 7, 8, 5, 6, seed=5)
    assert len({tuple(r.tolist()) for r in d["table"]}) == 5 and len({tuple(r.tolist()) for r in d["code"]}) == 6


@pytest.mark.parametrize("B,W,C", [(2, 5, 24), (1, 7, 64)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_column_sum_data_shows_the_order(dtype, B, W, C):
    """A condition on the inputs: with three rows or more the descending sum differs from the ascending one in at least a tenth of
    the outputs, and with a whole trip of four so does the pairwise sum.  (One row has no order; two rows add to 0.f commutatively.)"""
    for H in G.COLUMN_SUM_H:
        x = E.order_data(B, H, W, C, seed=1000 + 100 * H + C, dtype=dtype)
        up, down, pair = E.colsum_ascending(x), E.colsum_descending(x), E.colsum_pairwise(x, G.COLUMN_SUM_ROWS)
        np.testing.assert_allclose(up.numpy(), x.double().sum(1).numpy(), rtol=0, atol=2e-6 * float(x.float().abs().sum(1).max()))
        share = lambda a: float((a.view(torch.int32) != up.view(torch.int32)).float().mean())       # noqa: E731
        if H >= 3:
            assert share(down) >= 0.1, (H, share(down))
        else:
            assert share(down) == 0.0
        if H >= G.COLUMN_SUM_ROWS:
            assert share(pair) >= 0.1, (H, share(pair))
        else:
            assert share(pair) == 0.0


def test_column_sum_multi_trip_data_shows_the_order_too():
    B, H, W, C = G.column_sum_multi_trip_shape(F32)
    x = E.order_data(B, H, 64, C, seed=9)                                                    # the same draw rule at a sixty-fourth of the width
    up = E.colsum_ascending(x)
    assert float((E.colsum_descending(x).view(torch.int32) != up.view(torch.int32)).float().mean()) >= 0.1
    assert float((E.colsum_pairwise(x).view(torch.int32) != up.view(torch.int32)).float().mean()) >= 0.1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_integer_probe_is_exact_in_any_order(dtype):
    x = E.integer_data(2, 7, 3, 8, seed=29, dtype=dtype)
    assert torch.equal(x.float(), x.float().round()) and torch.equal(x.float().to(dtype).float(), x.float())
    assert int(x.float().abs().sum(1).max()) < 2 ** 24                                       # every partial sum in any order
    want = x.to(torch.int64).sum(1)
    for s in (E.colsum_ascending(x), E.colsum_descending(x), E.colsum_pairwise(x)):
        assert torch.equal(s.to(torch.int64), want)
    assert len(set(want.flatten().tolist())) > 40                                            # (48 outputs: a wrong index shows)


@pytest.mark.parametrize("n_bins", E.EDGE_BINS)
def test_edge_columns_are_exact(n_bins):
    f0, mean, u, bins = E.edge_case(n_bins)
    W = f0.shape[1] // 4
    b64, l64, u64, voiced = R.bins_f64(f0, W, n_bins, *E.EDGE_RANGE)
    b32, l32 = R.bins_f32(f0, W, n_bins, *E.EDGE_RANGE)
    assert np.log2(np.float64(64.0)) == 6.0 and np.float32(np.log2(512.0)) - np.float32(6.0) == 3.0
    assert np.array_equal(b64, bins) and np.array_equal(b32, bins) and np.array_equal(voiced, ~np.isnan(mean))
    assert np.array_equal(u64[voiced], u[voiced]) and np.array_equal(l64[voiced], mean[voiced]) and np.array_equal(l32[voiced], mean[voiced].astype(np.float32))
    exact = np.stack((E.EDGE_EXACT, E.EDGE_EXACT[::-1]))
    assert np.array_equal(l32[voiced & exact].astype(np.float64), mean[voiced & exact])
    assert (2 * u[voiced & exact] == np.round(2 * u[voiced & exact])).all()                  # integers and half-integers
    rest = u[~exact]                                                                         # the two thirds: far from every edge, and
    assert (np.abs(rest - np.round(rest)) > 0.3).all() and (np.rint(rest) != np.floor(rest)).any()      # one of them above a half
    by_name = {c[2].split(":")[0]: i for i, c in enumerate(E.EDGE_COLUMNS)}
    row = lambda k: (u[0, by_name[k]], bins[0, by_name[k]])                                  # noqa: E731
    assert row("u = 0") == (0, 1) and row("u = n_bins / 3, an integer") == (n_bins // 3, n_bins // 3 + 1)
    assert row("u = 2 n_bins / 3, an integer") == (2 * n_bins // 3, 2 * n_bins // 3 + 1) and row("u = n_bins") == (n_bins, n_bins)
    assert row("u = n_bins / 2") == (n_bins / 2, n_bins // 2 + 1) and row("u < 0") == (-n_bins / 3, 1) and row("u > n_bins") == (4 * n_bins / 3, n_bins)
    assert row("three voiced frames") == (n_bins // 3, n_bins // 3 + 1) and bins[0, by_name["one voiced frame"]] == 0
    # rint in place of floor, and a clamp one off, would each move one of these
    assert np.rint(n_bins / 2) + 1 != bins[0, by_name["u = n_bins / 2"]] or n_bins % 2 == 0


def test_voicing_case_covers_every_mask_at_every_cut():
    f0, frames, n, mean = E.voicing_case()
    assert f0.shape == (80, 13) and sorted(set(frames.tolist())) == [4, 5, 6, 7, 8]
    masks = {(int(frames[b]) - 4, tuple((f0[b, 4:8] > 0).tolist())) for b in range(80)}
    assert len(masks) == 80
    for b in range(80):
        assert n[b] == int((f0[b, 4:frames[b]] > 0).sum())
    assert (n[:16] == 0).all() and (n == 1).sum() > 0 and (n == 4).sum() == 1                 # cut 0: nothing below the end; mask 15 at cut 4
    # every subset of two or more frames has a mean of its own
    logs = np.log2(np.array(E.VOICING_HZ))
    means = [logs[[t for t in range(4) if m >> t & 1]].mean() for m in range(16) if bin(m).count("1") >= 2]
    assert len(set(means)) == 11
    b64, l64, u64, voiced = R.bins_f64(f0, 3, E.VOICING_BINS, *E.VOICING_RANGE, frames=frames)
    b32, l32 = R.bins_f32(f0, 3, E.VOICING_BINS, *E.VOICING_RANGE, frames=frames)
    assert np.array_equal(voiced[:, 1], n >= 2) and voiced[:, 0].all() and not voiced[:, 2].any()
    assert np.array_equal(b64, b32) and np.allclose(l64[:, 1][n >= 2], mean[n >= 2], rtol=0, atol=1e-15)
    u = u64[:, 1][n >= 2]
    assert (np.abs(u - np.round(u)) < 1e-12).sum() > 0 and ((np.abs(u - np.round(u)) < 1e-12) | (np.abs(u - np.round(u)) > 0.3)).all()
    nv = E.not_voiced_case()
    assert not (nv[0] > 0).any() and (nv[1] > 0).sum() == 6 and np.signbit(nv[0, 0]) and np.isnan(nv[0, 8])


@pytest.mark.parametrize("n_bins", [1, 32, 256])
@pytest.mark.parametrize("B,W,extra", G.F0_SHAPES)
def test_contour_references_stay_inside_the_caps(B, W, extra, n_bins):
    """For every launch of the GPU test: at most 1 % of the voiced columns undecided, and the fp32 restatement judged as the kernel
    will be -- so the judgement is one an fp32 evaluation of the rule passes."""
    T = 4 * W + extra
    f0 = G.contour_case(B, W, extra)
    assert abs(float((f0[:, :4 * W] == 0).mean()) - 0.3) < 0.05 and (f0[:, :4 * W][f0[:, :4 * W] > 0] < E.RANGE[0]).any() and (f0 > E.RANGE[1]).any()
    seen = []
    for k in range(E.frame_sets(B)):
        frames = E.ragged_frames(B, T, W, k)
        seen += frames.tolist()
        for aff in (None, E.affine_rows(B, seed=k)):
            ref = E.f0_reference(f0, W, n_bins, *E.RANGE, frames=frames, affine=aff)
            assert ref["undecided"].sum() <= 0.01 * ref["voiced"].sum()
            b32, l32 = R.bins_f32(f0, W, n_bins, *E.RANGE, frames=frames, affine=aff)
            G.judge(ref, b32, l32, (B, W, extra, n_bins, k))
    assert set(E.must_frames(T, W)) <= set(seen) and {m % 4 for m in E.must_frames(T, W)[4:8]} == {0, 1, 2, 3}
    ref = E.f0_reference(f0, W, n_bins, *E.RANGE)
    assert ref["undecided"].sum() <= 0.01 * ref["voiced"].sum() and ref["voiced"].sum() > 0.8 * B * W
    if n_bins > 1:
        assert ref["b64"].min() == 0 and ref["b64"].max() == n_bins and len(set(ref["b64"].flatten().tolist())) > 20


def test_refused_range_is_one_value_in_fp32_log2():
    """fmin < fmax, yet fl32(log2 fmin) == fl32(log2 fmax).  (100 and its fp32 successor are not such a pair: their logarithms
    round to neighbouring fp32 values; 101 and its successor are the first from 100 upwards.)"""
    lo, hi = E.one_value_range()
    assert lo < hi and np.float32(hi) == np.nextafter(np.float32(lo), np.float32(1e3))
    assert np.float32(np.log2(np.float64(np.float32(lo)))) == np.float32(np.log2(np.float64(np.float32(hi))))
    print("one-value range:", lo, hi)
