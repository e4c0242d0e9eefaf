"""GPU: the F0-conditioned decoder's kernels (csrc/f0_cond.hip) against their definitions: nsg_f0_bins against the fp64 definition
of tests/helpers/f0_cond_ref.py, nsg_add_cond and nsg_column_sum bit for bit against torch's fp32 arithmetic in the stated order,
and the table gradient (column sums scattered over the bins) against an fp64 scatter."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from tests.helpers import f0_cond_ref as R  # noqa: E402

DEV = "cuda:0"
SHAPES = [(2, 3, 5, 8), (2, 3, 5, 24), (1, 20, 7, 64), (2, 20, 8, 128)]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- nsg_f0_bins ------------------------------------------------------------------------------------------------------------
FRAMES = (26, 10, 3, 0)


def f0_case():
    """(4, 26) fp32: row 0 a full clip whose six columns hold 4, 3, 2, 1, 0 and 4 voiced frames, the last above fmax; row 1 ends
    inside column 2 (frames 8, 9 of 8 .. 11), its column 0 below fmin; row 2 has three frames, one column's; row 3 none.  Every frame
    past a clip's end is voiced in the data, so a kernel that ignores `frames` is caught."""
    rs = np.random.RandomState(5)
    f = rs.uniform(90.0, 400.0, size=(4, 26)).astype(np.float32)
    f[0, 4 + 1] = 0.0                                  # column 1: three voiced
    f[0, 8 + 0] = f[0, 8 + 3] = 0.0                    # column 2: two
    f[0, 12:16] = 0.0
    f[0, 12 + 2] = 210.0                               # column 3: one -> unvoiced
    f[0, 16:20] = 0.0                                  # column 4: none
    f[0, 20:24] = rs.uniform(520.0, 600.0, size=4)     # column 5: above fmax -> the top bin
    f[1, 0:4] = rs.uniform(50.0, 60.0, size=4)         # below fmin -> bin 1
    return f


AFFINE = np.array([[7.0, 1.25, 7.4], [6.0, 0.5, 7.0], [7.5, 1.0, 7.25], [7.0, 1.0, 7.0]], dtype=np.float32)


@pytest.mark.parametrize("n_bins", [1, 32])
@pytest.mark.parametrize("with_affine", [False, True])
def test_f0_bins_against_the_fp64_definition(n_bins, with_affine):
    f, W = f0_case(), 6
    aff = AFFINE if with_affine else None
    b64, l64, u64, voiced = R.bins_f64(f, W, n_bins, 65.0, 500.0, FRAMES, aff)
    dec = R.decided(u64)
    # the inputs themselves: every voiced-frame count, both clamps, and (the reference alone) at most 1 % undecided
    assert voiced.sum() == 8 and voiced[0].tolist() == [True, True, True, False, False, True] and voiced[1].tolist() == [True, True, True, False, False, False]
    assert voiced[2].tolist() == [True] + [False] * 5 and not voiced[3].any()
    undecided = voiced & ~dec
    assert undecided.sum() / voiced.sum() <= 0.01
    if not with_affine:
        assert b64[0, 5] == n_bins and b64[1, 0] == 1 and (u64[0, 5] > n_bins) and (u64[1, 0] < 0)
    fd = torch.from_numpy(f).to(DEV)
    ad = torch.from_numpy(aff).to(DEV) if with_affine else None
    bins, logf = ops.f0_bins(fd, W, n_bins, 65.0, 500.0, frames=list(FRAMES), affine=ad, want_logf=True)
    got_b, got_l = bins.cpu().numpy(), logf.cpu().numpy()
    assert bins.dtype == torch.int64 and tuple(bins.shape) == (4, W)
    assert np.array_equal(got_b[dec], b64[dec])
    assert np.abs(got_b - b64)[undecided].max(initial=0) <= 1
    assert (np.abs(got_l.astype(np.float64) - l64) <= 4 * np.spacing(np.abs(l64).astype(np.float32)))[voiced].all()
    # unvoiced columns and columns past the clip: bin 0 and +0.0
    assert not got_b[~voiced].any() and not got_l.view(np.int32)[~voiced].any()
    # the bins alone (no logf), frames already on the device, and a clip on its own: the same bits
    fr = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    assert torch.equal(ops.f0_bins(fd, W, n_bins, 65.0, 500.0, frames=fr, affine=ad), bins)
    for b in range(4):
        b1, l1 = ops.f0_bins(fd[b:b + 1].contiguous(), W, n_bins, 65.0, 500.0, frames=[FRAMES[b]], affine=None if ad is None else ad[b:b + 1].contiguous(),
                             want_logf=True)
        assert torch.equal(b1[0], bins[b]) and torch.equal(bits(l1[0]), bits(logf[b]))
    # frames = None: the whole row, here for the clip that is whole anyway
    assert torch.equal(ops.f0_bins(fd[:1].contiguous(), W, n_bins, 65.0, 500.0, affine=None if ad is None else ad[:1].contiguous()), bins[:1])


# ---- nsg_add_cond -----------------------------------------------------------------------------------------------------------
def cond_inputs(B, H, W, C, n_rows, K=11, used=None):
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + C)
    x = torch.randn(B, H, W, C, generator=g)
    code = torch.randn(K, C, generator=g)
    idx = torch.randint(0, K, (B, H, W), generator=g)
    clip = torch.randn(B, C, generator=g)
    table = torch.randn(n_rows, C, generator=g)
    used = n_rows if used is None else used
    bins = (torch.arange(B * W) % used)[torch.randperm(B * W, generator=g)].view(B, W)
    assert sorted(set(bins.flatten().tolist())) == list(range(used))         # every bin value in use occurs
    return x, code, idx, clip, table, bins


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_add_cond_is_bitwise_the_stated_fp32_arithmetic(B, H, W, C):
    x, code, idx, clip, table, bins = cond_inputs(B, H, W, C, n_rows=5)
    d = {k: v.to(DEV) for k, v in dict(x=x, code=code, idx=idx, clip=clip, table=table, bins=bins).items()}
    for with_clip, gather, relu, dtype in itertools.product((True, False), (False, True), (False, True), (torch.float32, torch.bfloat16)):
        if dtype == torch.bfloat16 and C % 8:
            continue
        src = code[idx] if gather else x
        want = src + clip[:, None, None, :] if with_clip else src
        want = want + table[bins][:, None, :, :]
        want = (torch.relu(want) if relu else want).to(dtype)
        got = ops.add_cond(d["code"] if gather else d["x"], d["table"], d["bins"], idx=d["idx"] if gather else None,
                           clip_rows=d["clip"] if with_clip else None, relu=relu, out_dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == (B, H, W, C)
        assert torch.equal(bits(got.cpu()), bits(want)), (with_clip, gather, relu, dtype)
    # a zero table, rows mode: ops.add_per_clip's bits (x + row, then the store type's rounding)
    zero = torch.zeros_like(d["table"])
    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16 and C % 8:
            continue
        a = ops.add_cond(d["x"], zero, d["bins"], clip_rows=d["clip"], out_dtype=dtype)
        assert torch.equal(bits(a), bits(ops.add_per_clip(d["x"], d["clip"], out_dtype=dtype)))
    # a preallocated destination, and the latent rows given flat with their grid
    out = torch.empty(B, H, W, C, device=DEV)
    assert ops.add_cond(d["x"].view(-1, C), d["table"], d["bins"], clip_rows=d["clip"], out=out, grid=(B, H, W)) is out
    assert torch.equal(out.cpu(), (x + clip[:, None, None, :]) + table[bins][:, None, :, :])


def test_add_cond_refuses_the_fp32_vector_width_for_a_bf16_store():
    x, code, idx, clip, table, bins = (t.to(DEV) for t in cond_inputs(2, 3, 5, 12, n_rows=5))
    assert tuple(ops.add_cond(x, table, bins).shape) == (2, 3, 5, 12)
    with pytest.raises(RuntimeError, match="nsg_add_cond: C = 12 must be a multiple of 8"):
        ops.add_cond(x, table, bins, out_dtype=torch.bfloat16)


# ---- nsg_column_sum and the table gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_column_sum_is_bitwise_the_ascending_fp32_sum(B, H, W, C, dtype):
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C)).to(dtype)
    acc = torch.zeros(B, W, C)
    for h in range(H):
        acc = acc + x[:, h].float()
    xd = x.to(DEV)
    got = ops.column_sum(xd)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, W, C)
    assert torch.equal(bits(got.cpu()), bits(acc))
    assert torch.equal(bits(ops.column_sum(xd)), bits(got))


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_table_gradient_from_column_sums(B, H, W, C):
    """d loss / d table = the gradient summed over each column's latent rows, scattered over the bins; tolerance: the speaker
    table's in tests/test_gpu_model.py.  Two of the seven rows are absent from bins: their gradient is exactly zero."""
    n_rows = 7
    dz, _, _, _, _, bins = cond_inputs(B, H, W, C, n_rows=n_rows, used=5)
    want = torch.zeros(n_rows, C, dtype=torch.float64)
    want.index_add_(0, bins.view(-1), dz.double().sum(1).view(-1, C))
    cs = ops.column_sum(dz.to(DEV))
    got = ops.index_add_rows(bins.to(DEV).view(-1), cs.view(-1, C), n_rows).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-4 * float(want.abs().max()))
    assert float(got[5:].abs().max()) == 0.0
    # ... and the clip rows' gradient from the same column sums is the per-clip sum over all latent pixels
    per_clip = ops.clip_colsum(cs, B).cpu()
    np.testing.assert_allclose(per_clip.numpy(), dz.double().sum((1, 2)).numpy(), rtol=2e-4, atol=2e-4 * float(dz.double().sum((1, 2)).abs().max()))
