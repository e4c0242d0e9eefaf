"""GPU parity tests, op level: every C-ABI kernel against the oracle (oracle/ for the bit-exact VQ,
CPU PyTorch fp32 for floating-point kernels -- the same ATen ops the reference calls) on seeded
inputs, plus the committed golden vectors.  Tolerances are written at each comparison."""
import os

import ctypes
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from neural_sound_generation_amd.vector_quantization import vq, vq_st, codebook_lookup  # noqa: E402
from oracle import vqvae_oracle as O  # noqa: E402
import portable_rng  # noqa: E402

DEV = "cuda:0"


def gpu(t):
    return t.to(DEV).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ---------------------------------------------------------------------------------------------
# VQ
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 16, 37, 64, 128, 256])
def test_mfma_dot_is_an_fmaf_chain(D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(64, D, generator=g)
    e = torch.randn(96, D, generator=g) * 0.01
    a = ops.debug_dot(gpu(x), gpu(e), 0).cpu()
    b = ops.debug_dot(gpu(x), gpu(e), 1).cpu()
    assert torch.equal(a, b), f"MFMA dot differs from the fmaf chain in {(a != b).sum().item()} entries"


@pytest.mark.parametrize("D", [1, 7, 8, 16, 24, 37, 64, 96, 128, 256])
def test_rowsumsq_bitwise(D):
    g = torch.Generator().manual_seed(100 + D)
    v = torch.randn(517, D, generator=g)
    got = ops.rowsumsq(gpu(v)).cpu().numpy()
    assert np.array_equal(got, O.rowsumsq(v.numpy()))


@pytest.mark.parametrize("impl", ["mfma", "valu"])
def test_vq_fixtures_robust_and_ties(golden_dir, impl):
    g = golden(golden_dir, "vq_ops.npz")
    idx, codes, _ = ops.vq_forward(gpu(torch.from_numpy(g["f1.x"])), gpu(torch.from_numpy(g["f1.e"])), impl=impl)
    assert np.array_equal(idx.cpu().numpy(), g["f1.idx"])
    assert np.array_equal(codes.cpu().numpy(), g["f1.codes"])
    xb = torch.from_numpy(g["f1b.x"])
    idx, _, _ = ops.vq_forward(gpu(xb.view(-1, xb.shape[-1])), gpu(torch.from_numpy(g["f1b.e"])), impl=impl)
    assert np.array_equal(idx.cpu().numpy().reshape(g["f1b.idx"].shape), g["f1b.idx"])  # first index on ties
    idx, _, _ = ops.vq_forward(gpu(torch.from_numpy(g["f1c.x"])), gpu(torch.from_numpy(g["f1c.e"])), impl=impl)
    assert np.array_equal(idx.cpu().numpy(), g["f1c.idx"])


@pytest.mark.parametrize("tag", ["f2a", "f2b", "f2c", "f2d"])
@pytest.mark.parametrize("impl", ["mfma", "valu"])
def test_vq_fixtures_fragile_bit_exact(golden_dir, tag, impl):
    g = golden(golden_dir, "vq_ops.npz")
    N, D, K, seed = (int(v) for v in g[tag + ".shape"])
    x, e = portable_rng.vq_case(N, D, K, seed)
    idx, _, dmin = ops.vq_forward(gpu(torch.from_numpy(x)), gpu(torch.from_numpy(e)), want_dist=True, impl=impl)
    bad = int((idx.cpu().numpy() != g[tag + ".idx"]).sum())
    assert bad == 0, f"{bad}/{N} indices differ from the reference's"
    assert np.array_equal(dmin.cpu().numpy(), g[tag + ".dmin"])


@pytest.mark.parametrize("N,D,K", [(1, 128, 512), (7, 64, 128), (333, 128, 100), (129, 37, 24), (1000, 8, 3), (4096, 256, 1000)])
def test_vq_ragged_against_oracle(N, D, K):
    x, e = portable_rng.vq_case(N, D, K, 900 + N)
    want, wdist = O.vq_indices(x, e, return_dist=True)
    idx, codes, dmin = ops.vq_forward(gpu(torch.from_numpy(x)), gpu(torch.from_numpy(e)), want_dist=True)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dmin.cpu().numpy(), wdist)
    assert np.array_equal(codes.cpu().numpy(), e[want])


@pytest.mark.parametrize("N,D,K", [(81920, 128, 512), (655360, 128, 512), (163840, 256, 8192)])
def test_vq_full_size_properties(N, D, K):
    """BASELINE sizes (configs[1]: 16 clips and the bench's 128 clips of 80x1024 -> 81920 / 655360 rows, K=512, D=128; configs[3]:
    32 clips, K=8192, D=256): size-independent checks -- run-to-run determinism, the gathered code is the indexed row, the
    reported minimum is attained by the reported index, quantising the codes themselves is idempotent (exact search and bf16x3), and
    a 4096-row sample is bit-exact against the oracle."""
    x, e = portable_rng.vq_case(N, D, K, 4242)
    xg, eg = gpu(torch.from_numpy(x)), gpu(torch.from_numpy(e))
    idx, codes, dmin = ops.vq_forward(xg, eg, want_dist=True)
    idx2, _, dmin2 = ops.vq_forward(xg, eg, want_dist=True)
    assert torch.equal(idx, idx2) and torch.equal(dmin, dmin2)
    assert torch.equal(codes, eg[idx])
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    sel = np.arange(0, N, N // 4096)
    want, wdist = O.vq_indices(x[sel], e, return_dist=True)
    assert np.array_equal(idx.cpu().numpy()[sel], want)
    assert np.array_equal(dmin.cpu().numpy()[sel], wdist)
    # idempotence: a code vector quantises to a code at zero distance from it (itself, unless the codebook holds duplicates)
    for impl in ("mfma", "bf16x3"):
        again = ops.vq_forward(codes, eg, impl=impl)[0]
        assert torch.equal(eg[again], codes), impl
    del x, xg, codes


@pytest.mark.parametrize("impl", ["mfma", "bf16x3"])
def test_vq_sliced_search_equals_the_unsplit_search(impl):
    """BASELINE configs[3]'s search (81920 rows, K = 8192, D = 256): 640 row blocks do not fill the 512 resident slots evenly,
    so the exact (fp32) search (one block per CU at D = 256: 640 blocks on 256 slots) cuts the codebook into slices and a combine pass takes the first minimum over them.  The result
    must be the unsplit search's, bit for bit: the first 65536 rows alone are 512 blocks = two full rounds (one slice: the unsplit kernel) and a
    row's result does not depend on the other rows; the exact search is also held to the CPU oracle on a sample.  (The bf16x3
    search stays unsplit -- it runs at the bf16 pipe's power-limited rate already, and the three slice arguments cost it its
    third block per CU: 311 -> 391 us at K = 512; measured, reverted -- the same properties are checked on it.)"""
    N, D, K = 81920, 256, 8192
    x, e = portable_rng.vq_case(N, D, K, 777)
    xg, eg = gpu(torch.from_numpy(x)), gpu(torch.from_numpy(e))
    kw = dict(impl=impl, want_dist=True)
    if impl == "bf16x3":
        kw["codes_bf16"] = "relu"
    full = ops.vq_forward(xg, eg, **kw)
    again = ops.vq_forward(xg, eg, **kw)
    head = ops.vq_forward(xg[:65536].contiguous(), eg, **kw)
    for a, b, c in zip(full, again, head):
        assert torch.equal(a, b), "the sliced search must be bitwise reproducible"
        assert torch.equal(a[:65536], c), "sliced and unsplit launches disagree"
    idx, codes, dmin = full[:3]
    assert torch.equal(codes, eg[idx]) and int(idx.min()) >= 0 and int(idx.max()) < K
    if impl == "bf16x3":
        assert torch.equal(full[3], torch.relu(eg[idx]).to(torch.bfloat16))
    else:
        sel = np.arange(0, N, 40)
        want, wdist = O.vq_indices(x[sel], e, return_dist=True)
        assert np.array_equal(idx.cpu().numpy()[sel], want)
        assert np.array_equal(dmin.cpu().numpy()[sel], wdist)


@pytest.mark.parametrize("N,D,K", [(640, 64, 128), (1000, 128, 512), (333, 24, 40), (256, 256, 1000), (129, 8, 7)])
def test_vq_bf16x3_search_is_near_exact(golden_dir, N, D, K):
    """The bf16 mode's search (split operands on the bf16 pipe): not bit-exact by design -- the code it picks must be
    a true nearest code up to its stated distance error (~2^-16 relative), and on well-separated data the very same."""
    g = torch.Generator().manual_seed(N + D + K)
    x = torch.randn(N, D, generator=g)
    e = torch.randn(K, D, generator=g)
    idx, codes, dmin = ops.vq_forward(gpu(x), gpu(e), want_dist=True, impl="bf16x3")
    idx = idx.cpu()
    d = torch.cdist(x.double(), e.double()) ** 2
    true_min, true_idx = d.min(dim=1)
    picked = d[torch.arange(N), idx]
    scale = (x.double().norm(dim=1) ** 2 + (e.double().norm(dim=1) ** 2).max())
    assert float(((picked - true_min) / scale).max()) <= 1e-4          # a nearest code within the error bound
    assert float((idx == true_idx).float().mean()) >= 0.99              # separated data: the same code
    assert torch.equal(codes.cpu(), e[idx])                             # gathered rows are the fp32 codebook rows
    assert float(((dmin.cpu().double() - picked) / scale).abs().max()) <= 1e-4
    f = golden(golden_dir, "vq_ops.npz")                                # the robust fixture: identical indices
    i1, _, _ = ops.vq_forward(gpu(torch.from_numpy(f["f1.x"])), gpu(torch.from_numpy(f["f1.e"])), impl="bf16x3")
    assert np.array_equal(i1.cpu().numpy(), f["f1.idx"])


@pytest.mark.parametrize("N,D,K", [(5000, 128, 512), (777, 64, 100), (4096, 256, 37), (300, 24, 16)])
def test_index_add_rows_bf16x2(N, D, K):
    """Codebook scatter-add of the bf16 mode: rows split into bf16 hi + lo on the bf16 pipe; sums to ~2^-17, deterministic."""
    g = torch.Generator().manual_seed(N + K)
    idx = torch.randint(0, K, (N,), generator=g)
    rows = torch.randn(N, D, generator=g)
    want = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, rows.double())
    got, cnt = ops.index_add_rows(gpu(idx), gpu(rows), K, want_counts=True, impl="bf16x2")
    scale = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, rows.double().abs()).clamp_min(1e-6)
    assert float(((got.cpu().double() - want).abs() / scale).max()) <= 3e-5
    assert torch.equal(cnt.cpu(), torch.bincount(idx, minlength=K).float())
    got2 = ops.index_add_rows(gpu(idx), gpu(rows), K, impl="bf16x2")
    assert torch.equal(got, got2), "must be bitwise reproducible"


def test_vq_lean_path_pieces():
    """The bf16 mode's quantiser without an fp32 copy of z_q: the search's bf16 (ReLU'd) code rows, the losses with q read
    from the codebook through the indices, and the codebook gradient from per-code sums -- each against the materialised
    form (bit-identical loss and dz: the same arithmetic on the same values)."""
    g = torch.Generator().manual_seed(11)
    N, D, K = 5000, 128, 512
    z = gpu(torch.randn(N, D, generator=g))
    e = gpu(torch.randn(K, D, generator=g) * 0.8)
    idx, codes, _, lp = ops.vq_forward(z, e, want_codes=True, impl="bf16x3", codes_bf16="relu")
    assert torch.equal(codes, e[idx])
    assert torch.equal(lp, torch.relu(codes).bfloat16())
    _, _, _, lp2 = ops.vq_forward(z, e, want_codes=False, impl="bf16x3", codes_bf16="plain")
    assert torch.equal(lp2, codes.bfloat16())
    add = gpu(torch.randn(N, D, generator=g)).bfloat16()
    for gd, a in ((torch.float32, None), (torch.bfloat16, add)):
        loss1, dz1, dq1 = ops.vq_losses(z, codes, dz_scale=0.25, dq_scale=1.0, dz_add=a, grad_dtype=gd)
        loss2, dz2 = ops.vq_losses_indexed(z, e, idx, dz_scale=0.25, dz_add=a, grad_dtype=gd)
        assert torch.equal(dz1, dz2)
        assert abs(float(loss1) - float(loss2)) <= 1e-6 * abs(float(loss1))
    # codebook gradient: 2/numel * (n_k e_k - s_k) against the scatter of dq (1e-5 of the largest entry)
    want = ops.index_add_rows(idx, dq1, K)
    s_, n_ = ops.index_add_rows(idx, z, K, want_counts=True)
    got = (e * n_.unsqueeze(1) - s_) * (2.0 / z.numel())
    _close(got.cpu(), want.cpu(), tol=1e-5, what="codebook gradient from per-code sums")


def test_vq_operator_surface(golden_dir):
    g = golden(golden_dir, "vq_ops.npz")
    x = gpu(torch.from_numpy(g["st.x"])).requires_grad_(True)
    e = gpu(torch.from_numpy(g["st.e"])).requires_grad_(True)
    codes, idx = vq_st(x, e)
    (codes * gpu(torch.from_numpy(g["st.w"]))).sum().backward()
    assert np.array_equal(idx.cpu().numpy(), g["st.idx"])
    assert np.array_equal(codes.detach().cpu().numpy(), g["st.codes"])
    assert np.array_equal(x.grad.cpu().numpy(), g["st.gx"])                       # straight-through: exact copy
    np.testing.assert_allclose(e.grad.cpu().numpy(), g["st.ge"], rtol=1e-6, atol=1e-6)  # fp32 sum order
    xb = gpu(torch.from_numpy(g["f1b.x"]))
    out = vq(xb, gpu(torch.from_numpy(g["f1b.e"])))
    assert out.shape == xb.shape[:-1] and out.dtype == torch.int64
    with pytest.raises(RuntimeError):
        xi = gpu(torch.from_numpy(g["st.x"])).requires_grad_(True)
        vq(xi, e).float().sum().backward()
    # codebook lookup = index_select with gradient to the codebook (models.py:137)
    e2 = gpu(torch.from_numpy(g["st.e"])).requires_grad_(True)
    look = codebook_lookup(e2, idx)
    (look * gpu(torch.from_numpy(g["st.w"]))).sum().backward()
    np.testing.assert_allclose(e2.grad.cpu().numpy(), g["st.ge"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("impl", ["f32", "sorted"])
@pytest.mark.parametrize("N,D,K", [(300, 16, 24), (5000, 64, 128), (20000, 128, 512), (3000, 256, 1000), (4, 16, 7), (1000, 32, 101),
                                   (9000, 256, 8192), (70000, 128, 512), (4097, 8, 3), (130, 512, 40)])
def test_index_add_rows_and_counts(N, D, K, impl):
    """index_add_ (vector_quantization.py:60-61): the one-hot GEMM and the sorted segment sum (stable counting sort of the row
    indices, each code's rows added in row order).  Skewed (a third of the rows on one code: many sort rounds per 64 rows, many
    128-row chunks per code), codes without rows, block boundaries of the sort (4096 rows), wide rows (D = 512)."""
    g = torch.Generator().manual_seed(N)
    idx = torch.randint(0, K, (N,), generator=g)
    idx[: N // 3] = min(5, K - 1)  # skewed: one hot code
    v = torch.randn(N, D, generator=g)
    want = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, v.double())
    assert impl != "sorted" or ops.index_add_sorted_supported(N, D, K)
    out, cnt = ops.index_add_rows(gpu(idx), gpu(v), K, want_counts=True, impl=impl)
    out2 = ops.index_add_rows(gpu(idx), gpu(v), K, impl=impl)
    assert torch.equal(out, out2), "index_add_rows must be bitwise reproducible"
    scale = float(want.abs().max())
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=1e-5, atol=2e-6 * scale + 1e-6)
    assert torch.equal(cnt.cpu(), torch.bincount(idx, minlength=K).float())
    if impl == "sorted":        # preallocated destinations (the EMA statistics live behind the gradient bucket), and sum order = row order:
        kp = (K + 63) // 64 * 64                            # (16-byte aligned views, as FusedTrainStep lays them out)
        buf = torch.full((kp + K * D,), float("nan"), device=DEV)
        ops.index_add_rows(gpu(idx), gpu(v), K, impl=impl, out=buf[kp:].view(K, D), counts=buf[:K])
        assert torch.equal(buf[kp:].view(K, D), out) and torch.equal(buf[:K], cnt)
        k = int(idx[-1])                                    # a sparse code: its rows added one by one in row order, exactly
        rows = (idx == k).nonzero().flatten()
        if rows.numel() <= 128 and D <= 256:
            acc = torch.zeros(D)
            ppr, rpi = D // 4, max(1, 64 // (D // 4))
            subs = [torch.zeros(D) for _ in range(rpi)]     # the kernel's lanes: row j of the chunk goes to sub-accumulator j % rpi
            for j, r in enumerate(rows.tolist()):
                subs[j % rpi] = subs[j % rpi] + v[r]
            for sacc in subs:
                acc = acc + sacc if sacc is not subs[0] else sacc.clone()
            assert torch.equal(out[k].cpu(), acc), "a code's rows are summed in row order"


def test_ema_update_against_oracle():
    K, D = 48, 16
    g = torch.Generator().manual_seed(5)
    w = torch.randn(K, D, generator=g)
    ema_n = torch.rand(K, generator=g) * 10
    ema_s = torch.randn(K, D, generator=g)
    z = torch.randn(700, D, generator=g)
    idx = torch.randint(0, K, (700,), generator=g)
    n, s = O.ema_stats(z, idx, K)
    w_ref, n_ref, s_ref = O.ema_update(w.clone(), ema_n.clone(), ema_s.clone(), n, s)
    sg, ng = ops.index_add_rows(gpu(idx), gpu(z), K, want_counts=True)
    np.testing.assert_allclose(sg.cpu().numpy(), s.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(ng.cpu(), n)
    wg, eng, esg = gpu(w), gpu(ema_n), gpu(ema_s)
    ops.vq_ema_update(wg, eng, esg, ng, sg)
    np.testing.assert_allclose(eng.cpu().numpy(), n_ref.numpy(), rtol=1e-6)
    np.testing.assert_allclose(esg.cpu().numpy(), s_ref.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(wg.cpu().numpy(), w_ref.numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# convolutions: forward / dgrad / wgrad against CPU torch autograd (fp32; rtol 2e-5 of the output scale)
# ---------------------------------------------------------------------------------------------
def _close(got, want, tol=2e-5, what=""):
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


CONV_CASES = [
    # (B, IH, IW, C_in, C_out, k, stride, pad, transposed, relu_in, tanh_out)
    (2, 10, 12, 8, 8, 3, 1, 1, False, True, False),     # ResBlock 3x3 with fused ReLU
    (2, 10, 12, 16, 16, 1, 1, 0, False, False, False),  # ResBlock 1x1
    (3, 20, 24, 16, 16, 4, 2, 1, False, False, False),  # encoder.3
    (2, 11, 15, 16, 16, 4, 2, 1, False, False, False),  # encoder.3 with odd extents (T=31 path)
    (2, 6, 7, 16, 16, 4, 2, 1, True, True, False),      # decoder.3 with fused ReLU
    (2, 20, 16, 1, 16, 4, 2, 1, False, False, False),   # encoder.0 (single input channel)
    (2, 20, 31, 1, 8, 4, 2, 1, False, False, False),    # encoder.0 odd width
    (2, 10, 8, 16, 1, 4, 2, 1, True, False, True),      # decoder.6 (single output channel) + tanh
    (2, 20, 32, 64, 64, 3, 1, 1, False, True, False),   # 64 channels (config 1)
    (1, 20, 64, 128, 128, 3, 1, 1, False, True, False), # 128 channels (full)
    (1, 8, 16, 256, 256, 4, 2, 1, False, False, False), # 256 channels: two column tiles
    (1, 4, 8, 256, 256, 4, 2, 1, True, False, False),
    (2, 20, 70, 128, 128, 3, 1, 1, False, False, False),  # 128 channels, no fused ReLU: the row-strip weight gradient (64-pixel strips + a ragged one)
    (2, 14, 40, 128, 128, 4, 2, 1, False, False, False),  # ... its stride-2 form (32-pixel strips in fp32)
    (2, 9, 9, 96, 96, 3, 1, 1, False, False, False),    # channel count not a power of two
    (2, 12, 20, 16, 32, 7, 1, 3, False, False, False),  # 7x7 'same' (the PixelCNN prior's first layer, models.py:291)
    (1, 9, 11, 8, 8, 5, 1, 2, False, False, False),     # 5x5
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[str(c) for c in CONV_CASES])
def test_conv_forward_dgrad_wgrad(case):
    B, IH, IW, Ci, Co, k, s, p, tr, relu_in, tanh_out = case
    g = torch.Generator().manual_seed(hash(case) % 10007)
    x = torch.randn(B, Ci, IH, IW, generator=g, requires_grad=True)
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    w = (torch.randn(*wshape, generator=g) * 0.1).requires_grad_(True)
    b = (torch.randn(Co, generator=g) * 0.1).requires_grad_(True)
    xin = F.relu(x) if relu_in else x
    y = F.conv_transpose2d(xin, w, b, stride=s, padding=p) if tr else F.conv2d(xin, w, b, stride=s, padding=p)
    if tanh_out:
        y = torch.tanh(y)
    dy = torch.randn(y.shape, generator=g)
    # gradients w.r.t. the conv's own input (after the fused relu) and pre-tanh output
    if tanh_out:
        y_lin = F.conv_transpose2d(xin, w, b, stride=s, padding=p) if tr else F.conv2d(xin, w, b, stride=s, padding=p)
        gx, gw, gb = torch.autograd.grad(y_lin, [xin, w, b], dy) if relu_in else torch.autograd.grad(y_lin, [x, w, b], dy)
    else:
        y2 = y
        gx, gw, gb = torch.autograd.grad(y2, [xin if relu_in else x, w, b], dy)

    d = ops.conv_desc(B, IH, IW, Ci, Co, k, s, p, transposed=tr)
    assert (d.OH, d.OW) == tuple(y.shape[2:])
    wg = gpu(w.detach())
    wf, wd = ops.pack_weights(d, wg)
    flags = (ops.NSG_RELU_IN if relu_in else 0) | (ops.NSG_TANH_OUT if tanh_out else 0)
    xg = gpu(nhwc(x.detach()))
    yg = ops.conv_forward(d, xg, wf, gpu(b.detach()), flags=flags)
    _close(nchw(yg.cpu()), y.detach(), what="forward")
    dyg = gpu(nhwc(dy))
    dxg = ops.conv_dgrad(d, dyg, wd)
    _close(nchw(dxg.cpu()), gx, what="dgrad")
    if Ci > 1 and Co > 1:   # (dgrad + skip gradient) * ReLU mask in the dgrad store == the two separate kernels, bit for bit in fp32
        skip = torch.randn(dxg.shape, generator=g).to(DEV)
        rx = torch.relu(torch.randn(dxg.shape, generator=g)).to(DEV)
        fused = ops.conv_dgrad(d, dyg, wd, add=skip, relu_x=rx)
        assert torch.equal(fused, ops.relu_backward_add(skip, dxg, rx))
        assert torch.equal(ops.conv_dgrad(d, dyg, wd, relu_x=rx), ops.relu_backward_add(dxg, None, rx))
    dwg, dbg = ops.conv_wgrad(d, xg, dyg, wshape, flags=ops.NSG_RELU_IN if relu_in else 0)
    _close(dwg.cpu(), gw, what="wgrad")
    _close(dbg.cpu(), gb, what="bias grad")
    dwg2, _ = ops.conv_wgrad(d, xg, dyg, wshape, flags=ops.NSG_RELU_IN if relu_in else 0)
    assert torch.equal(dwg, dwg2), "wgrad must be bitwise reproducible"


RECT_CASES = [
    # (B, H, W, C_in, C_out, (kh, kw), (ph, pw)): output cropped to (H, W) -- the prior's masked stacks (models.py:238-252,268-273)
    (2, 9, 13, 16, 32, (4, 7), (3, 3)),    # vertical stack, kernel 7
    (2, 9, 13, 16, 32, (1, 4), (0, 3)),    # horizontal stack, kernel 7
    (2, 20, 24, 8, 16, (2, 3), (1, 1)),    # vertical stack, kernel 3
    (1, 6, 40, 8, 16, (1, 2), (0, 1)),     # horizontal stack, kernel 3
    (2, 7, 9, 8, 8, (3, 5), (1, 2)),       # a plain rectangular 'same' convolution
]


@pytest.mark.parametrize("case", RECT_CASES, ids=str)
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_rectangular_cropped_conv(case, bf):
    B, H, W, Ci, Co, (kh, kw), (ph, pw) = case
    g = torch.Generator().manual_seed(kh * 10 + kw)
    dt = torch.bfloat16 if bf else torch.float32

    def q(t):
        return t.to(dt).float()
    x = q(torch.randn(B, Ci, H, W, generator=g)).requires_grad_(True)
    w = q(torch.randn(Co, Ci, kh, kw, generator=g) * 0.2).requires_grad_(True)
    b = torch.randn(Co, generator=g).requires_grad_(True)
    y = F.conv2d(x, w, b, 1, (ph, pw))[:, :, :H, :W]
    dy = q(torch.randn(y.shape, generator=g))
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], dy)
    d = ops.conv_desc(B, H, W, Ci, Co, (kh, kw), 1, (ph, pw), dtype=dt, out_hw=(H, W))
    wf, wd = ops.pack_weights(d, gpu(w.detach()))
    xg, dyg = gpu(nhwc(x.detach())).to(dt), gpu(nhwc(dy)).to(dt)
    yg = ops.conv_forward(d, xg, wf, gpu(b.detach()))
    tol = 1e-2 if bf else 2e-5
    _close(nchw(yg.float().cpu()), y.detach(), tol=tol, what="forward")
    _close(nchw(ops.conv_dgrad(d, dyg, wd).float().cpu()), gx, tol=tol, what="dgrad")
    dwg, dbg = ops.conv_wgrad(d, xg, dyg, tuple(w.shape))
    _close(dwg.cpu(), gw, tol=2e-3 if bf else 2e-5, what="wgrad")
    _close(dbg.cpu(), gb, tol=1e-4, what="bias grad")


@pytest.mark.parametrize("case", [(2, 10, 12, 8, 8, 3, 1, 1, False), (2, 11, 15, 16, 16, 4, 2, 1, False), (2, 6, 7, 16, 16, 4, 2, 1, True),
                                  (2, 20, 31, 1, 8, 4, 2, 1, False), (1, 20, 64, 128, 128, 3, 1, 1, False), (1, 8, 16, 256, 256, 4, 2, 1, False),
                                  (3, 5, 9, 64, 64, 4, 2, 1, True)], ids=str)
def test_conv_forward_with_fused_bn_statistics(case):
    """conv + BatchNorm training statistics in one call == conv, then nsg_bn_stats (and == ATen)."""
    B, IH, IW, Ci, Co, k, s, p, tr = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Ci, IH, IW, generator=g)
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    w = torch.randn(*wshape, generator=g) * 0.2
    b = torch.randn(Co, generator=g)
    y = F.conv_transpose2d(x, w, b, stride=s, padding=p) if tr else F.conv2d(x, w, b, stride=s, padding=p)
    rm, rv = torch.zeros(Co), torch.ones(Co)
    F.batch_norm(y, rm, rv, None, None, True, 0.1, 1e-5)
    d = ops.conv_desc(B, IH, IW, Ci, Co, k, s, p, transposed=tr)
    wf, _ = ops.pack_weights(d, gpu(w))
    rmg, rvg = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
    yg, mean, invstd = ops.conv_forward_bnstats(d, gpu(nhwc(x)), wf, gpu(b), running_mean=rmg, running_var=rvg)
    _close(nchw(yg.cpu()), y, what="forward")
    want_mean = y.double().mean(dim=(0, 2, 3))
    want_var = y.double().var(dim=(0, 2, 3), unbiased=False)
    std = float(want_var.sqrt().max())          # a mean is only meaningful to ~1e-6 of the column's spread
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=1e-5, atol=2e-6 * std + 1e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), (1.0 / torch.sqrt(want_var + 1e-5)).numpy(), rtol=2e-5)
    np.testing.assert_allclose(rmg.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=2e-7 * std + 1e-6)
    np.testing.assert_allclose(rvg.cpu().numpy(), rv.numpy(), rtol=2e-5, atol=1e-6)
    m2, i2 = ops.bn_stats(yg, Co)
    np.testing.assert_allclose(mean.cpu().numpy(), m2.cpu().numpy(), rtol=1e-5, atol=2e-6 * std + 1e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), i2.cpu().numpy(), rtol=1e-5)


BF16_CASES = [
    (2, 10, 12, 16, 16, 3, 1, 1, False, True),     # ResBlock 3x3 + fused ReLU
    (2, 10, 12, 16, 16, 1, 1, 0, False, False),    # 1x1
    (2, 11, 15, 16, 24, 4, 2, 1, False, False),    # stride-2, odd extents
    (2, 6, 7, 16, 16, 4, 2, 1, True, True),        # transposed + fused ReLU
    (2, 20, 16, 1, 16, 4, 2, 1, False, False),     # single input channel (fp32 image in)
    (2, 10, 8, 16, 1, 4, 2, 1, True, False),       # single output channel (fp32 image out)
    (1, 20, 64, 128, 128, 3, 1, 1, False, True),   # full width
    (1, 8, 16, 256, 256, 4, 2, 1, False, False),   # two column tiles
    (1, 4, 8, 128, 128, 4, 2, 1, True, False),
]


@pytest.mark.parametrize("case", BF16_CASES, ids=str)
def test_conv_bf16_mode(case):
    """bf16 storage / bf16 MFMA with fp32 accumulation.  Reference: fp32 ATen on the SAME bf16-rounded
    operands, so the only differences are accumulation order and the final rounding of the output to
    bf16 (relative 2^-8); gradients w.r.t. weights stay fp32."""
    B, IH, IW, Ci, Co, k, s, p, tr, relu_in = case
    g = torch.Generator().manual_seed(sum(case[:9]))
    bf = torch.bfloat16

    def rnd(t):   # round to bf16 values, keep fp32 storage
        return t.to(bf).float()

    x = rnd(torch.randn(B, Ci, IH, IW, generator=g)) if Ci > 1 else torch.randn(B, Ci, IH, IW, generator=g)
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    w = torch.randn(*wshape, generator=g) * 0.1
    b = torch.randn(Co, generator=g) * 0.1
    # what the packed images hold: bf16, except that the stencil kernels of the single-channel layers (the forward
    # of a C_in=1 conv, the data gradient of a C_out=1 transposed conv) read the fp32 weights and the fp32 image
    wq = rnd(w) if Ci > 1 else w
    xr = x.clone().requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    xin = F.relu(xr) if relu_in else xr
    y = F.conv_transpose2d(xin, wr, br, stride=s, padding=p) if tr else F.conv2d(xin, wr, br, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g)
    dyq = rnd(dy) if Co > 1 else dy
    gx, gw, gb = torch.autograd.grad(y, [xin if Ci > 1 else xr, wr, br], dyq)
    if Co == 1:   # data gradient with the unrounded weights
        xin2 = (F.relu(x) if relu_in else x).clone().requires_grad_(True)
        gx, = torch.autograd.grad(F.conv_transpose2d(xin2, w, b, stride=s, padding=p), [xin2], dyq)

    d = ops.conv_desc(B, IH, IW, Ci, Co, k, s, p, transposed=tr, dtype=bf)
    wf, wd = ops.pack_weights(d, gpu(w))
    xg = gpu(nhwc(x)).to(bf) if Ci > 1 else gpu(nhwc(x))
    yg = ops.conv_forward(d, xg, wf, gpu(b), flags=ops.NSG_RELU_IN if relu_in else 0)
    assert yg.dtype == (bf if Co > 1 else torch.float32)
    _close(nchw(yg.float().cpu()), y.detach(), tol=1e-2 if Co > 1 else 2e-3, what="forward")
    if Co > 1:
        yf = ops.conv_forward(d, xg, wf, gpu(b), flags=(ops.NSG_RELU_IN if relu_in else 0) | ops.NSG_OUT_F32)
        assert yf.dtype == torch.float32
        _close(nchw(yf.cpu()), y.detach(), tol=2e-3, what="forward (fp32 out)")
    dyg = gpu(nhwc(dyq)).to(bf) if Co > 1 else gpu(nhwc(dyq))
    dxg = ops.conv_dgrad(d, dyg, wd)
    _close(nchw(dxg.float().cpu()), gx, tol=1e-2, what="dgrad")
    dwg, dbg = ops.conv_wgrad(d, xg, dyg, wshape, flags=ops.NSG_RELU_IN if relu_in else 0)
    assert dwg.dtype == torch.float32
    _close(dwg.cpu(), gw, tol=2e-3, what="wgrad")
    _close(dbg.cpu(), gb, tol=1e-4, what="bias grad")


PATCH_CASES = [
    # (B, IH, IW, C_in, C_out, k, stride, transposed): the shapes gemm_patch.hip implements (bf16, C_in % 64 == 0, C_out % 128 == 0)
    (2, 20, 64, 128, 128, 3, 1, False),     # the ResBlock 3x3: 5 x 2 tiles per clip
    (3, 9, 45, 64, 128, 3, 1, False),       # ragged in both directions, one channel chunk
    (1, 4, 32, 256, 256, 3, 1, False),      # exactly one tile, four chunks, two column tiles
    (2, 40, 128, 128, 128, 4, 2, False),    # encoder.3: parity planes
    (2, 22, 30, 128, 128, 4, 2, False),     # odd output extents (11 x 15)
    (2, 11, 15, 64, 128, 4, 2, False),      # odd INPUT extents (the T = 31 path)
    (2, 20, 64, 128, 128, 4, 2, True),      # decoder.3: four parity classes per tile
    (3, 6, 7, 64, 128, 4, 2, True),         # ragged, small
    (1, 5, 33, 256, 256, 4, 2, True),       # four chunks x four classes = 16 jobs
]


@pytest.mark.parametrize("case", PATCH_CASES, ids=str)
def test_patch_staged_conv_kernel(case):
    """gemm_patch.hip (input patch + halo staged once in LDS, weights straight to registers) against (a) fp32 ATen on the same
    bf16-rounded operands and (b) gemm_gather.hip's kernel on the same tensors -- same products, different summation order,
    so outputs agree to the rounding of the bf16 store.  Forward with bias (+ ReLU for the consumer) and the data gradient
    with the fused skip-gradient add and ReLU mask; every launch twice (bitwise reproducible)."""
    from neural_sound_generation_amd import _lib
    B, IH, IW, Ci, Co, k, s, tr = case
    p = 1
    g = torch.Generator().manual_seed(sum(case[:7]) + 17 * int(tr))
    bf = torch.bfloat16
    x = torch.randn(B, Ci, IH, IW, generator=g).to(bf).float()
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    w = (torch.randn(*wshape, generator=g) * 0.05)
    wq = w.to(bf).float()
    b = torch.randn(Co, generator=g) * 0.1
    xr = x.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wq, b, stride=s, padding=p) if tr else F.conv2d(xr, wq, b, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g).to(bf).float()
    gx, = torch.autograd.grad(y, [xr], dy)
    d = ops.conv_desc(B, IH, IW, Ci, Co, k, s, p, transposed=tr, dtype=bf)
    wf, wd = ops.pack_weights(d, gpu(w))
    xg = gpu(nhwc(x)).to(bf)
    dyg = gpu(nhwc(dy)).to(bf)
    skip = torch.randn(B, IH, IW, Ci, generator=g).to(bf).to(DEV)
    rx = torch.relu(torch.randn(B, IH, IW, Ci, generator=g)).to(bf).to(DEV)

    def run():
        return (ops.conv_forward(d, xg, wf, gpu(b)), ops.conv_forward(d, xg, wf, gpu(b), flags=ops.NSG_RELU_OUT),
                ops.conv_dgrad(d, dyg, wd), ops.conv_dgrad(d, dyg, wd, add=skip, relu_x=rx))
    new = run()
    again = run()
    dw_new, _ = ops.conv_wgrad(d, xg, dyg, wshape, want_bias=False)      # gemm_wgrad_strip.hip when both channel counts are multiples of 128
    dw_again, _ = ops.conv_wgrad(d, xg, dyg, wshape, want_bias=False)
    with _lib.use_diag() as lib:        # the diagnostics build of the same sources: switch to gemm_gather.hip / the per-tap kernels
        lib.nsg_debug_set_patch_gemm(0)
        lib.nsg_debug_set_wgrad_strip(0)
        try:
            old = run()
            dw_old, _ = ops.conv_wgrad(d, xg, dyg, wshape, want_bias=False)
        finally:
            lib.nsg_debug_set_patch_gemm(1)
            lib.nsg_debug_set_wgrad_strip(1)
    # BatchNorm batch statistics from the store phase of the wave-private epilogue (one record per workgroup; of the values AS
    # STORED, rounded to bf16) == a pass over the stored tensor
    rmg, rvg = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
    ys, mean, invstd = ops.conv_forward_bnstats(d, xg, wf, gpu(b), running_mean=rmg, running_var=rvg)
    assert torch.equal(ys, new[0]), "the statistics variant must store the same tensor"
    m2, i2 = ops.bn_stats(ys, Co)
    spread = float((1.0 / i2).max())
    np.testing.assert_allclose(mean.cpu().numpy(), m2.cpu().numpy(), rtol=1e-5, atol=2e-6 * spread + 1e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), i2.cpu().numpy(), rtol=2e-5)
    ysf = nchw(ys.float().cpu()).double()
    np.testing.assert_allclose(mean.cpu().numpy(), ysf.mean(dim=(0, 2, 3)).numpy(), rtol=1e-5, atol=2e-6 * spread + 1e-6)
    M_ = ysf.numel() // Co
    np.testing.assert_allclose(rvg.cpu().numpy(), (0.9 + 0.1 * ysf.var(dim=(0, 2, 3), unbiased=True)).numpy() if M_ > 1 else rvg.cpu().numpy(), rtol=5e-5)
    ys2, mean2, invstd2 = ops.conv_forward_bnstats(d, xg, wf, gpu(b))
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2), "the statistics must be bitwise reproducible"
    # weight gradient: fp32 out, against ATen on the same bf16-rounded operands and against the per-tap kernel
    wr = wq.clone().requires_grad_(True)
    yw = F.conv_transpose2d(x, wr, None, stride=s, padding=p) if tr else F.conv2d(x, wr, None, stride=s, padding=p)
    gw, = torch.autograd.grad(yw, [wr], dy)
    assert torch.equal(dw_new, dw_again), "the weight gradient must be bitwise reproducible"
    _close(dw_new.cpu(), gw, tol=2e-3, what="wgrad")
    _close(dw_new.cpu(), dw_old.cpu(), tol=1e-5, what="wgrad vs the per-tap kernel (same bf16 products, fp32 sums in another order)")
    for a, c in zip(new, again):
        assert torch.equal(a, c), "the patch-staged kernel must be bitwise reproducible"
    _close(nchw(new[0].float().cpu()), y.detach(), tol=1e-2, what="forward")
    _close(nchw(new[1].float().cpu()), torch.relu(y.detach()), tol=1e-2, what="forward + ReLU")
    _close(nchw(new[2].float().cpu()), gx, tol=1e-2, what="dgrad")
    want = (gx + nchw(skip.float().cpu())) * (nchw(rx.float().cpu()) > 0)
    _close(nchw(new[3].float().cpu()), want, tol=1e-2, what="dgrad + add + mask")
    for a, c, what in zip(new, old, ("forward", "forward + ReLU", "dgrad", "dgrad + add + mask")):
        a, c = a.float(), c.float()
        scale = float(c.abs().max())
        # one bf16 ulp at the value's own magnitude (2^-8 relative) plus the fp32 accumulation-order noise
        assert bool(((a - c).abs() <= c.abs() * 2.0 ** -7 + 1e-5 * scale).all()), f"{what}: differs from gemm_gather beyond a bf16 ulp"
        assert float((a != c).float().mean()) < 0.05, f"{what}: more than 5 % of the outputs round differently"


@pytest.mark.parametrize("k,s,tr", [(3, 1, False), (4, 2, False), (4, 2, True)], ids=["3x3", "4x4s2", "4x4s2T"])
def test_conv_full_size_batch_independence(k, s, tr):
    """The bench's full size (128 clips; low-resolution grid 20 x 256, D = 128, bf16: 168 / 671 MB tensors, the 31-bit offsets'
    range) through a size-independent property: a clip's output does not depend on what else is in the batch -- forward, the data
    gradient with its fused add + mask and the BatchNorm statistics variant give, for the first, a middle and the last clip, the
    bits a launch on that clip alone gives; the weight gradient of the batch is the sum of the clips' (fp32 sums, 1e-3 of scale)."""
    B, C, bf = 128, 128, torch.bfloat16
    IH, IW = (20, 256) if (s == 1 or tr) else (40, 512)
    g = torch.Generator(device=DEV).manual_seed(k + s + int(tr))
    d = ops.conv_desc(B, IH, IW, C, C, k, s, 1, transposed=tr, dtype=bf)
    d1 = ops.conv_desc(1, IH, IW, C, C, k, s, 1, transposed=tr, dtype=bf)
    wshape = (C, C, k, k)
    w = torch.randn(*wshape, device=DEV, generator=g) * 0.05
    b = torch.randn(C, device=DEV, generator=g) * 0.1
    wf, wd = ops.pack_weights(d, w)
    x = torch.randn(B, IH, IW, C, device=DEV, generator=g).to(bf)
    dy = torch.randn(B, d.OH, d.OW, C, device=DEV, generator=g).to(bf)
    skip = torch.randn(B, IH, IW, C, device=DEV, generator=g).to(bf)
    rx = torch.relu(torch.randn(B, IH, IW, C, device=DEV, generator=g)).to(bf)
    y = ops.conv_forward(d, x, wf, b)
    ys, _, _ = ops.conv_forward_bnstats(d, x, wf, b)
    dx = ops.conv_dgrad(d, dy, wd, add=skip, relu_x=rx)
    assert torch.equal(y, ys)
    dw, _ = ops.conv_wgrad(d, x, dy, wshape, want_bias=False)
    for c in (0, 77, B - 1):
        sl = slice(c, c + 1)
        assert torch.equal(ops.conv_forward(d1, x[sl].contiguous(), wf, b), y[sl]), c
        assert torch.equal(ops.conv_dgrad(d1, dy[sl].contiguous(), wd, add=skip[sl].contiguous(), relu_x=rx[sl].contiguous()), dx[sl]), c
    acc = torch.zeros_like(dw, dtype=torch.float64)
    for c in range(0, B, 16):        # 8 chunks of 16 clips
        d16 = ops.conv_desc(16, IH, IW, C, C, k, s, 1, transposed=tr, dtype=bf)
        acc += ops.conv_wgrad(d16, x[c:c + 16].contiguous(), dy[c:c + 16].contiguous(), wshape, want_bias=False)[0].double()
    _close(dw.double().cpu(), acc.cpu(), tol=1e-3, what="weight gradient of the batch vs the sum over its chunks")


def test_conv_rejects_unsupported_geometry():
    from neural_sound_generation_amd._lib import NsgError
    d = ops.conv_desc(1, 8, 8, 6, 8, 3, 1, 1)  # C_in not a multiple of 4
    with pytest.raises(NsgError):
        ops.pack_weights(d, gpu(torch.zeros(8, 6, 3, 3)))
    with pytest.raises(NsgError):
        ops.vq_forward(gpu(torch.zeros(4, 300)), gpu(torch.zeros(8, 300)))  # D > 256
    with pytest.raises(NsgError):
        ops.vq_forward(torch.zeros(4, 8), torch.zeros(8, 8))  # CPU tensors: no fallback


# ---------------------------------------------------------------------------------------------
# batch norm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,relu,res", [(2, 8, 5, 6, True, False), (3, 16, 20, 16, False, True), (2, 64, 20, 64, True, False),
                                              (2, 128, 40, 128, True, False), (1, 256, 20, 32, False, True), (2, 96, 7, 9, True, False)])
def test_batchnorm_train_forward_backward(B, C, H, W, relu, res):
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(B, C, H, W, generator=g) * 2.0 + 3.0).requires_grad_(True)   # mean >> 0: exercises the variance path
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.2).requires_grad_(True)
    r = torch.randn(B, C, H, W, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
    if relu:
        y = F.relu(y)
    if res:
        y = y + F.relu(r)
    dy = torch.randn(y.shape, generator=g)
    gx, gg, gb = torch.autograd.grad(y, [x, gamma, beta], dy)

    xg = gpu(nhwc(x.detach()))
    rmg, rvg = gpu(rm), gpu(rv)
    mean, invstd = ops.bn_stats(xg, C, rmg, rvg)
    np.testing.assert_allclose(rmg.cpu().numpy(), rm_ref.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rvg.cpu().numpy(), rv_ref.numpy(), rtol=1e-5, atol=1e-6)
    yg = ops.bn_apply(xg, mean, invstd, gpu(gamma.detach()), gpu(beta.detach()), relu=relu,
                      residual=gpu(nhwc(r)) if res else None, relu_residual=res)
    _close(nchw(yg.cpu()), y.detach(), tol=1e-5, what="bn forward")
    # backward w.r.t. the BN input: the residual branch passes dy through untouched
    ybn = ops.bn_apply(xg, mean, invstd, gpu(gamma.detach()), gpu(beta.detach()), relu=relu) if relu else None
    dxg, dgg, dbg = ops.bn_backward(xg, ybn, gpu(nhwc(dy)), mean, invstd, gpu(gamma.detach()))
    _close(nchw(dxg.cpu()), gx, tol=3e-5, what="bn dx")
    # the fused column sum of dx (bias gradient of the conv in front): same dx, plus sum over rows
    cs = torch.empty(C, device=DEV)
    dxg2, _, _ = ops.bn_backward(xg, ybn, gpu(nhwc(dy)), mean, invstd, gpu(gamma.detach()), dx_colsum=cs)
    _close(dxg2.cpu(), dxg.cpu(), tol=1e-6, what="bn dx (colsum variant)")
    if relu:   # ReLU mask re-derived from x with the forward's arithmetic: the same mask, bit for bit
        dxg3, dgg3, dbg3 = ops.bn_backward(xg, None, gpu(nhwc(dy)), mean, invstd, gpu(gamma.detach()), relu_beta=gpu(beta.detach()))
        assert torch.equal(dxg3, dxg) and torch.equal(dgg3, dgg) and torch.equal(dbg3, dbg)
    want_cs = dxg.double().sum(dim=(0, 1, 2)).cpu()
    assert float((cs.cpu().double() - want_cs).abs().max()) <= 1e-5 * float(dxg.abs().sum(dim=(0, 1, 2)).max()) + 1e-7
    _close(dgg.cpu(), gg, tol=3e-5, what="bn dgamma")
    _close(dbg.cpu(), gb, tol=3e-5, what="bn dbeta")


@pytest.mark.parametrize("B,H,W,C", [(2, 8, 12, 8), (3, 80, 64, 128), (2, 20, 260, 48), (1, 6, 130, 256), (2, 4, 4, 4),
                                     (2, 20, 260, 96), (1, 6, 130, 32), (2, 8, 12, 64), (2, 10, 300, 128),
                                     (2, 80, 256, 256),         # C = 256 (BASELINE configs[3]): 8 waves per block in the bf16 mode
                                     (4, 80, 1024, 128)])       # the last: BASELINE configs[1]'s image extent
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_c1conv_bn_relu_fused_layer(B, H, W, C, bf):
    """encoder.0-2 (Conv2d(1, C, 4, 2, 1) -> BatchNorm2d -> ReLU, src/models.py:165-167) as one operator whose conv output is
    never stored: against CPU PyTorch autograd (1e-5 forward, 3e-5 gradients, relative to the largest reference value) and
    against the unfused operators of this library (fp32: the same conv values bit for bit, so the same mask and results
    to rounding of the statistics' summation order)."""
    g = torch.Generator().manual_seed(B * 1000 + C + W)
    img = torch.randn(B, 1, H, W, generator=g) * 0.7 + 0.3
    w = (torch.randn(C, 1, 4, 4, generator=g) * 0.3).requires_grad_(True)
    b = (torch.randn(C, generator=g) * 0.2).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.2).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y = F.relu(F.batch_norm(F.conv2d(img, w, b, 2, 1), rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5))
    dy = torch.randn(y.shape, generator=g)
    gw, gb, gg, gbe = torch.autograd.grad(y, [w, b, gamma, beta], dy)

    dt = torch.bfloat16 if bf else torch.float32
    imgg = gpu(img.view(B, H, W))
    wg, bg, gag, beg = gpu(w.detach()), gpu(b.detach()), gpu(gamma.detach()), gpu(beta.detach())
    rmg, rvg = gpu(rm), gpu(rv)
    yg, mean, invstd = ops.c1conv_bn_relu_forward(imgg, wg, bg, gag, beg, rmg, rvg, training=True, out_dtype=dt)
    np.testing.assert_allclose(rmg.cpu().numpy(), rm_ref.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rvg.cpu().numpy(), rv_ref.numpy(), rtol=1e-5, atol=1e-6)
    _close(nchw(yg.float().cpu()), y.detach(), tol=1e-2 if bf else 1e-5, what="fused layer forward")
    dyg = gpu(nhwc(dy)).to(dt)
    dw, dbias, dgm, dbt = ops.c1conv_bn_relu_backward(imgg, wg, bg, gag, beg, mean, invstd, dyg)
    tol = 2e-2 if bf else 3e-5           # bf16: dy, dh and the patch operand of the weight-gradient MFMA carry 8 bits (as every bf16 wgrad)
    _close(dw.cpu(), gw, tol=tol, what="fused layer dw")
    _close(dgm.cpu(), gg, tol=tol, what="fused layer dgamma")
    _close(dbt.cpu(), gbe, tol=tol, what="fused layer dbeta")
    # the conv bias sits in front of a BatchNorm: its true gradient is zero up to rounding
    assert float(dbias.abs().max()) <= 1e-4 * float(dyg.float().abs().sum(dim=(0, 1, 2)).max()) + 1e-6

    if bf and ops.bn_relu_c1convt_supported(torch.bfloat16, C):
        # the bf16 layer works from the image's tap moments (statistics without a pass over h, backward in one pass over dy):
        # against the two-pass forms of the same kernels (nsg_debug_set_c1_moments(0)): statistics to 1e-5, weight gradient to 2e-2
        # (the two-pass weight gradient rounds dh to bf16, the one-pass form multiplies the exact bf16 dy)
        from neural_sound_generation_amd import _lib
        with _lib.use_diag() as lib:        # the diagnostics build carries the switch; the product library has only the one-pass form
            lib.nsg_debug_set_c1_moments(0)
            try:
                y2, mean2, invstd2 = ops.c1conv_bn_relu_forward(imgg, wg, bg, gag, beg, training=True, out_dtype=dt)
                dw2p, dbias2p, dgm2p, dbt2p = ops.c1conv_bn_relu_backward(imgg, wg, bg, gag, beg, mean, invstd, dyg)
            finally:
                lib.nsg_debug_set_c1_moments(1)
        np.testing.assert_allclose(mean.cpu().numpy(), mean2.cpu().numpy(), rtol=1e-5, atol=5e-6)      # (h itself carries 2^-17 per product
        np.testing.assert_allclose(invstd.cpu().numpy(), invstd2.cpu().numpy(), rtol=1e-5)             #  in the two-pass form)
        _close(dgm.cpu(), dgm2p.cpu(), tol=1e-5, what="one-pass dgamma vs two-pass")
        _close(dbt.cpu(), dbt2p.cpu(), tol=1e-5, what="one-pass dbeta vs two-pass")
        _close(dw.cpu(), dw2p.cpu(), tol=2e-2, what="one-pass dw vs two-pass")

    # eval mode: statistics are inputs
    em, ei = ops.bn_eval_stats(rmg, rvg)
    ye, _, _ = ops.c1conv_bn_relu_forward(imgg, wg, bg, gag, beg, training=False, mean=em, invstd=ei, out_dtype=dt)
    y_eval = F.relu(F.batch_norm(F.conv2d(img, w, b, 2, 1), rm_ref, rv_ref, gamma, beta, False, 0.1, 1e-5)).detach()
    _close(nchw(ye.float().cpu()), y_eval, tol=1e-2 if bf else 1e-5, what="fused layer eval forward")

    if not bf:   # against the unfused chain of this library, given the SAME statistics: identical values
        d = ops.conv_desc(B, H, W, 1, C, 4, 2, 1)
        wf, _ = ops.pack_weights(d, wg, want_dgrad=False)
        h = ops.conv_forward(d, imgg.view(B, H, W, 1), wf, bg)
        a = ops.bn_apply(h, mean, invstd, gag, beg, relu=True)
        assert torch.equal(a, yg), "recomputed conv values differ from the stored ones"
        dh, dg2, db2 = ops.bn_backward(h, None, dyg, mean, invstd, gag, relu_beta=beg)
        _close(dgm.cpu(), dg2.cpu(), tol=1e-5, what="dgamma vs unfused")
        _close(dbt.cpu(), db2.cpu(), tol=1e-5, what="dbeta vs unfused")
        dw2, _ = ops.conv_wgrad(d, imgg.view(B, H, W, 1), dh, (C, 1, 4, 4), want_bias=False)
        _close(dw.cpu(), dw2.cpu(), tol=2e-5, what="dw vs unfused")


@pytest.mark.parametrize("B,H,W,C,T", [(2, 5, 150, 64, 300), (3, 40, 64, 128, 131), (1, 3, 70, 32, 143)])
def test_fused_output_layer_with_reconstruction_loss(B, H, W, C, T):
    """nsg_bn_relu_c1convt_forward_mse = the fused output layer (with Tanh) + nsg_mse_padded + nsg_tanh_backward in one pass over
    the tap products: the same image bit for bit, the loss to the order of its double sums, the gradient at the Tanh's input to
    one rounding; with a target wider than the image (the reference zero-pads x_tilde on the host, train.py:118-127)."""
    # (tests/test_gpu_fused_output_envelope.py::test_loss_form covers these checks strictly: fp64, T = 2W | 2W + 1 | 2W + 37, poison, canaries)
    g = torch.Generator().manual_seed(B + W + C)
    u = gpu(torch.randn(B, H, W, C, generator=g) * 1.2 + 0.3).bfloat16()
    w = gpu(torch.randn(C, 1, 4, 4, generator=g) * 0.2)
    bias = gpu(torch.randn(1, generator=g) * 0.1)
    gamma, beta = gpu(torch.rand(C, generator=g) + 0.5), gpu(torch.randn(C, generator=g) * 0.3)
    mean, invstd = ops.bn_stats(u, C, None, None)
    target = gpu(torch.rand(B, 2 * H, T, 1, generator=g))
    xt = ops.bn_relu_c1convt_forward(u, mean, invstd, gamma, beta, w, bias, tanh=True)
    loss_ref, dxt = ops.mse_padded(xt, target, B * 2 * H, 2 * W, T)
    dpre_ref = ops.tanh_backward(dxt, xt)
    loss, dpre, img = ops.bn_relu_c1convt_forward_mse(u, mean, invstd, gamma, beta, w, bias, target, want_image=True)
    assert torch.equal(img, xt)
    np.testing.assert_allclose(loss.cpu().numpy(), loss_ref.cpu().numpy(), rtol=1e-6)
    _close(dpre.cpu(), dpre_ref.cpu(), tol=1e-6, what="gradient at the Tanh's input")
    db = torch.empty(1, device=DEV)
    loss2, dpre2, none = ops.bn_relu_c1convt_forward_mse(u, mean, invstd, gamma, beta, w, bias, target, dbias=db)
    assert none is None and torch.equal(loss2, loss) and torch.equal(dpre2, dpre)
    np.testing.assert_allclose(float(db.cpu()), float(dpre.double().sum().cpu()), rtol=1e-5, atol=1e-9)     # the transposed conv's bias gradient
    # float64 CPU statement of the loss on the stored image
    pad = torch.zeros(B, 2 * H, T, dtype=torch.float64)
    pad[:, :, :2 * W] = xt.cpu().double().view(B, 2 * H, 2 * W)
    np.testing.assert_allclose(float(loss.cpu()), float(((pad - target.cpu().double().view(B, 2 * H, T)) ** 2).mean()), rtol=1e-6)


def test_c1conv_tap_moments_with_a_large_image_mean():
    """The bf16 input layer takes its BatchNorm statistics and weight gradient from the image's tap moments (c1_mfma.hip).  The
    moments are taken about a shift (a sample mean of the image), so an image whose mean dwarfs its spread (mean^2 / var =
    3600 here) costs no accuracy: against float64 CPU PyTorch."""
    B, H, W, C = 2, 40, 128, 64
    g = torch.Generator().manual_seed(7)
    img = torch.randn(B, 1, H, W, generator=g) * 0.05 + 3.0
    w = torch.randn(C, 1, 4, 4, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.2
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    h = F.conv2d(img.double(), w.double(), b.double(), 2, 1)
    mean_ref, var_ref = h.mean(dim=(0, 2, 3)), h.var(dim=(0, 2, 3), unbiased=False)
    mom = torch.empty(ops.C1_MOMENTS, dtype=torch.float64, device=DEV)
    y, mean, invstd = ops.c1conv_bn_relu_forward(gpu(img.view(B, H, W)), gpu(w), gpu(b), gpu(gamma), gpu(beta), training=True,
                                                 out_dtype=torch.bfloat16, moments=mom)
    np.testing.assert_allclose(mean.cpu().numpy(), mean_ref.float().numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), (1.0 / torch.sqrt(var_ref + 1e-5)).float().numpy(), rtol=2e-5)
    # and the one-pass backward built on the same moments, against float64 autograd of the same layer
    wd, bd, gd, bed = (t.double().requires_grad_(True) for t in (w, b, gamma, beta))
    yd = F.relu(F.batch_norm(F.conv2d(img.double(), wd, bd, 2, 1), None, None, gd, bed, True, 0.1, 1e-5))
    dy = torch.randn(yd.shape, generator=g).bfloat16()
    gw, gg, gbe = torch.autograd.grad(yd, [wd, gd, bed], dy.double())
    dw, dbias, dgm, dbt = ops.c1conv_bn_relu_backward(gpu(img.view(B, H, W)), gpu(w), gpu(b), gpu(gamma), gpu(beta), mean, invstd,
                                                      gpu(nhwc(dy.float())).bfloat16(), moments=mom)
    _close(dgm.cpu(), gg.float(), tol=2e-2, what="dgamma")
    _close(dbt.cpu(), gbe.float(), tol=2e-2, what="dbeta")
    _close(dw.cpu(), gw.float(), tol=3e-2, what="dw")       # (the bf16 image operand of the weight-gradient MFMA: 2^-9 of a mean-3 image)


@pytest.mark.parametrize("B,H,W,C", [(2, 8, 12, 32), (3, 40, 64, 128), (2, 10, 130, 96), (1, 3, 70, 64), (2, 5, 150, 128),
                                     (2, 5, 150, 256), (2, 40, 512, 256),    # C = 256 (BASELINE configs[3])
                                     (4, 40, 512, 128)])        # the last: BASELINE configs[1]'s decoder extent
def test_bn_relu_c1convt_fused_output_layer(B, H, W, C):
    """decoder.4-7 (BatchNorm2d -> ReLU -> ConvTranspose2d(C, 1, 4, 2, 1) -> Tanh, src/models.py:180-183) as one operator on bf16
    tensors, against CPU PyTorch autograd on the same bf16-rounded input.  The operator rounds relu(bn(u)) and the conv
    weights to bf16 on their way into the MFMA (as the separate bf16 operators do) and stores du as bf16: 1e-2 of the largest
    reference value; the image-sized outputs see the bf16 products averaged over C channels: 4e-3."""
    # (the comparisons with CPU autograd are covered strictly by tests/test_gpu_fused_output_envelope.py: fp64, derived bounds, no exclusions)
    g = torch.Generator().manual_seed(B * 100 + C + W)
    u = (torch.randn(B, C, H, W, generator=g) * 1.5 + 0.5).bfloat16().float().requires_grad_(True)
    w = (torch.randn(C, 1, 4, 4, generator=g) * 0.2).requires_grad_(True)
    b = (torch.randn(1, generator=g) * 0.1).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.3).requires_grad_(True)
    pre = F.conv_transpose2d(F.relu(F.batch_norm(u, None, None, gamma, beta, True, 0.1, 1e-5)), w, b, 2, 1)
    dy = torch.randn(pre.shape, generator=g)
    gu, gw, gb, gg, gbe = torch.autograd.grad(pre, [u, w, b, gamma, beta], dy)

    ug = gpu(nhwc(u.detach())).bfloat16()
    assert ops.bn_relu_c1convt_supported(torch.bfloat16, C) and not ops.bn_relu_c1convt_supported(torch.float32, C)
    mean, invstd = ops.bn_stats(ug, C, None, None)
    wg, bg, gag, beg = gpu(w.detach()), gpu(b.detach()), gpu(gamma.detach()), gpu(beta.detach())
    y_pre = ops.bn_relu_c1convt_forward(ug, mean, invstd, gag, beg, wg, bg, tanh=False)
    _close(nchw(y_pre.cpu()), pre.detach(), tol=4e-3, what="fused output layer forward")
    y_t = ops.bn_relu_c1convt_forward(ug, mean, invstd, gag, beg, wg, bg, tanh=True)
    assert torch.equal(y_t, torch.tanh(y_pre)) or float((y_t - torch.tanh(y_pre)).abs().max()) <= 2e-6
    dyg = gpu(dy.view(B, 2 * H, 2 * W))
    cs = torch.empty(C, device=DEV)
    du, dw, dbias, dgm, dbt = ops.bn_relu_c1convt_backward(ug, mean, invstd, gag, beg, wg, dyg, du_colsum=cs)
    # column sums of du (bias gradient of the conv in front of the BatchNorm; mathematically zero): against the fp32 values
    # before du's bf16 rounding -- bounded by the rounding of the stored du
    assert float((cs.cpu() - du.float().sum(dim=(0, 1, 2)).cpu()).abs().max()) <= 2e-2 * float(du.float().abs().sum(dim=(0, 1, 2)).max())
    # du: elements whose pre-activation sits within rounding of the ReLU threshold may take the other branch (fp32 statistics
    # summed in another order); they are excluded from the element-wise bound and must be rare
    t_ref = F.batch_norm(u.detach(), None, None, gamma.detach(), beta.detach(), True, 0.1, 1e-5)
    safe = t_ref.abs() > 1e-4
    assert float((~safe).float().mean()) < 1e-3
    _close(nchw(du.float().cpu()) * safe, gu * safe, tol=1e-2, what="fused output layer du")
    # (the sums see the same threshold elements: each one that flips moves a sum by its whole O(1) term -> 2e-2)
    _close(dw.cpu(), gw, tol=2e-2, what="fused output layer dw")
    _close(dgm.cpu(), gg, tol=2e-2, what="fused output layer dgamma")
    _close(dbt.cpu(), gbe, tol=2e-2, what="fused output layer dbeta")
    _close(dbias.cpu(), gb, tol=1e-5, what="fused output layer dbias")
    # against the separate operators of this library on the same tensors (they store a and da as bf16): same tolerance class
    d6 = ops.conv_desc(B, H, W, C, 1, 4, 2, 1, transposed=True, dtype=torch.bfloat16)
    wf6, wd6 = ops.pack_weights(d6, wg)
    a = ops.bn_apply(ug, mean, invstd, gag, beg, relu=True)
    y2 = ops.conv_forward(d6, a, wf6, bg, flags=0)
    _close(y_pre.cpu(), y2.cpu(), tol=2e-3, what="forward vs separate operators")
    dw2, _ = ops.conv_wgrad(d6, a, dyg.view(B, 2 * H, 2 * W, 1), (C, 1, 4, 4))
    _close(dw.cpu(), dw2.cpu(), tol=3e-3, what="dw vs separate operators")     # (two different bf16 roundings of a and da: 2.1e-3 seen at C = 256)


@pytest.mark.parametrize("B,H,W,C", [(2, 10, 12, 32), (3, 20, 64, 128), (1, 7, 37, 64), (2, 5, 130, 64), (4, 20, 256, 128),
                                     (33, 20, 256, 128),        # more tiles than persistent blocks (1320 > 512)
                                     (1, 7, 37, 256), (2, 20, 256, 256), (7, 20, 256, 256)])   # C = 256: the weights-in-registers kernel
                                                                # (259 rows: ragged; 160 tiles < 256 blocks; 560 tiles: 2-3 per block)
def test_resblock_1x1_conv_with_batchnorm_in_the_operand_staging(B, H, W, C):
    """nsg_bn_relu_conv1x1_* / nsg_bn_backward_conv1x1_dgrad / nsg_bn_backward_sums (bf16): against the separate operators of
    this library on the same tensors (which store the intermediate tensors as bf16 too: differences are single bf16
    roundings of O(1) values accumulated over C products -> 4e-3 of the largest value) and against CPU PyTorch."""
    # (the bit-for-bit contracts and the fp32 comparison are covered strictly, at every boundary M, by tests/test_gpu_fused_1x1_envelope.py)
    g = torch.Generator().manual_seed(C + W)
    M = B * H * W
    x = gpu(torch.randn(B, H, W, C, generator=g) * 1.3 + 0.4).bfloat16()
    w = gpu(torch.randn(C, C, 1, 1, generator=g) * 0.15)
    b = gpu(torch.randn(C, generator=g) * 0.1)
    gamma, beta = gpu(torch.rand(C, generator=g) + 0.5), gpu(torch.randn(C, generator=g) * 0.3)
    assert ops.bn_relu_conv1x1_supported(torch.bfloat16, C) and not ops.bn_relu_conv1x1_supported(torch.bfloat16, 96)
    mean, invstd = ops.bn_stats(x, C, None, None)
    d = ops.conv_desc(B, H, W, C, C, 1, 1, 0, dtype=torch.bfloat16)
    wf, wd = ops.pack_weights(d, w)
    a = ops.bn_apply(x, mean, invstd, gamma, beta, relu=True)
    y_ref = ops.conv_forward(d, a, wf, b)
    y = ops.bn_relu_conv1x1_forward(x, mean, invstd, gamma, beta, w, b)
    rm, rv = gpu(torch.randn(C, generator=g) * 0.1), gpu(torch.rand(C, generator=g) + 0.5)
    rm2, rv2 = rm.clone(), rv.clone()
    y_s, my, iy = ops.bn_relu_conv1x1_forward_bnstats(x, mean, invstd, gamma, beta, w, b, rm, rv)
    assert torch.equal(y_s, y)
    my_ref, iy_ref = ops.bn_stats(y, C, rm2, rv2)      # statistics from the store phase = a separate pass over y (summation order aside)
    np.testing.assert_allclose(my.cpu().numpy(), my_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(iy.cpu().numpy(), iy_ref.cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(rm.cpu().numpy(), rm2.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), rv2.cpu().numpy(), rtol=1e-5, atol=1e-6)
    _close(y.float().cpu(), y_ref.float().cpu(), tol=8e-3, what="fused 1x1 forward vs separate operators")
    # CPU fp32 reference of the same math on the bf16-rounded input
    xa = torch.relu((x.float().cpu() - mean.cpu()) * (invstd.cpu() * gamma.cpu()) + beta.cpu())
    y_cpu = xa.reshape(M, C) @ w.cpu().reshape(C, C).t() + b.cpu()
    _close(y.float().cpu().reshape(M, C), y_cpu, tol=1e-2, what="fused 1x1 forward vs fp32")

    dy = gpu(torch.randn(B, H, W, C, generator=g)).bfloat16()
    dw_ref, _ = ops.conv_wgrad(d, a, dy, (C, C, 1, 1), want_bias=False)
    dw = ops.bn_relu_conv1x1_wgrad(x, mean, invstd, gamma, beta, dy)
    _close(dw.cpu(), dw_ref.cpu(), tol=2e-3, what="fused 1x1 wgrad vs separate operators")

    # the second BatchNorm's backward + the 1x1 conv's data gradient
    h = y_ref
    m2, i2 = ops.bn_stats(h, C, None, None)
    g2 = gpu(torch.rand(C, generator=g) + 0.5)
    cs_ref = torch.empty(C, device=DEV)
    dh_ref, dg_ref, db_ref = ops.bn_backward(h, None, dy, m2, i2, g2, dx_colsum=cs_ref)
    dx_ref = ops.conv_dgrad(d, dh_ref, wd)
    dg, db = ops.bn_backward_sums(h, dy, m2, i2, g2)
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    cs = torch.empty(C, device=DEV)
    dh, dx = ops.bn_backward_conv1x1_dgrad(h, dy, m2, i2, g2, dg, db, w, dh_colsum=cs)
    _close(dh.float().cpu(), dh_ref.float().cpu(), tol=8e-3, what="fused dh vs bn_backward")
    _close(dx.float().cpu(), dx_ref.float().cpu(), tol=1e-2, what="fused dx vs separate operators")
    assert float((cs - cs_ref).abs().max()) <= 2e-3 * float(dh_ref.float().abs().sum(dim=(0, 1, 2)).max()) + 1e-5
    # ... with the sums of the BatchNorm + ReLU in front (x, mean, invstd, gamma, beta) formed while dx is written: the same
    # dx, and what nsg_bn_backward_sums gives on (x, that dx); then the apply half alone = bn_backward's dx
    dh_b, dx_b, pdg, pdb = ops.bn_backward_conv1x1_dgrad(h, dy, m2, i2, g2, dg, db, w, prev=(x, mean, invstd, gamma, beta))
    assert torch.equal(dx_b, dx) and torch.equal(dh_b, dh)
    pdg_ref, pdb_ref = ops.bn_backward_sums(x, dx, mean, invstd, gamma, relu_beta=beta)
    _close(pdg.cpu(), pdg_ref.cpu(), tol=1e-5, what="dgamma of the BatchNorm in front")
    _close(pdb.cpu(), pdb_ref.cpu(), tol=1e-5, what="dbeta of the BatchNorm in front")
    dxx_ref, _, _ = ops.bn_backward(x, None, dx, mean, invstd, gamma, relu_beta=beta)
    dxx = ops.bn_backward_apply(x, dx, mean, invstd, gamma, pdg_ref, pdb_ref, relu_beta=beta)
    assert torch.equal(dxx, dxx_ref)
    # ... and with the conv's weight gradient in the same pass (C = 128): the same dx bit for bit (same operands, same MFMA
    # chain), the same sums, and dw = what the weight-gradient kernel gives on (x, the bf16 dh) up to the order of the fp32 sums
    assert ops.bn_backward_conv1x1_dgrad_wgrad_supported(torch.bfloat16, C) == (C == 128)
    if C == 128:
        cs2 = torch.empty(C, device=DEV)
        dx_f, dw_f, pdg_f, pdb_f = ops.bn_backward_conv1x1_dgrad_wgrad(h, dy, m2, i2, g2, dg, db, w, (x, mean, invstd, gamma, beta), dh_colsum=cs2)
        assert torch.equal(dx_f, dx)
        _close(pdg_f.cpu(), pdg.cpu(), tol=1e-5, what="fused backward: dgamma of the BatchNorm in front")
        _close(pdb_f.cpu(), pdb.cpu(), tol=1e-5, what="fused backward: dbeta of the BatchNorm in front")
        assert float((cs2 - cs).abs().max()) <= 1e-5 * float(dh.float().abs().sum(dim=(0, 1, 2)).max()) + 1e-6    # (sums of a zero-mean tensor)
        dw_sep = ops.bn_relu_conv1x1_wgrad(x, mean, invstd, gamma, beta, dh)
        _close(dw_f.cpu(), dw_sep.cpu(), tol=2e-5, what="fused backward: dw vs the weight-gradient kernel on the stored dh")
        dx_g, dw_g, _, _ = ops.bn_backward_conv1x1_dgrad_wgrad(h, dy, m2, i2, g2, dg, db, w, (x, mean, invstd, gamma, beta))
        assert torch.equal(dx_g, dx_f) and torch.equal(dw_g, dw_f)      # run to run


def test_batchnorm_eval():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, 6, 5, generator=g)
    rm, rv = torch.randn(16, generator=g) * 0.1, torch.rand(16, generator=g) + 0.5
    gamma, beta = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g)
    y = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)
    mean, invstd = ops.bn_eval_stats(gpu(rm), gpu(rv))
    yg = ops.bn_apply(gpu(nhwc(x)), mean, invstd, gpu(gamma), gpu(beta))
    _close(nchw(yg.cpu()), y, tol=1e-5, what="bn eval")


# ---------------------------------------------------------------------------------------------
# element-wise, losses, optimiser
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 1001])
def test_elementwise(n):
    g = torch.Generator().manual_seed(n)
    a, b, x = (torch.randn(n, generator=g) for _ in range(3))
    np.testing.assert_array_equal(ops.relu_backward_add(gpu(a), gpu(b), gpu(x)).cpu().numpy(), ((a + b) * (x > 0)).numpy())
    np.testing.assert_array_equal(ops.relu_backward_add(gpu(a), None, gpu(x)).cpu().numpy(), (a * (x > 0)).numpy())
    y = torch.tanh(x)
    np.testing.assert_allclose(ops.tanh_backward(gpu(a), gpu(y)).cpu().numpy(), (a * (1 - y * y)).numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(ops.add(gpu(a), gpu(b)).cpu().numpy(), (a + b).numpy())


@pytest.mark.parametrize("rows,wa,wc", [(160, 64, 64), (160, 28, 31), (6, 1020, 1023)])
def test_mse_padded(rows, wa, wc):
    g = torch.Generator().manual_seed(rows + wa)
    a = torch.rand(rows, wa, generator=g, requires_grad=True)
    c = torch.rand(rows, wc, generator=g)
    loss = F.mse_loss(F.pad(a, (0, wc - wa)), c)
    (ga,) = torch.autograd.grad(loss, [a])
    lg, dag = ops.mse_padded(gpu(a.detach()), gpu(c), rows, wa, wc)
    np.testing.assert_allclose(lg.item(), loss.item(), rtol=1e-6)
    np.testing.assert_allclose(dag.cpu().numpy(), ga.numpy(), rtol=1e-5, atol=1e-9)


def test_vq_losses():
    g = torch.Generator().manual_seed(9)
    z = torch.randn(2, 20, 16, 16, generator=g, requires_grad=True)
    q = (torch.randn(2, 20, 16, 16, generator=g) * 0.1).requires_grad_(True)
    ste = torch.randn(2, 20, 16, 16, generator=g)
    beta = 0.25
    l_vq = F.mse_loss(q, z.detach())
    l_c = F.mse_loss(z, q.detach())
    gz, gq = torch.autograd.grad(l_vq + beta * l_c, [z, q])
    lg, dz, dq = ops.vq_losses(gpu(z.detach()), gpu(q.detach()), dz_scale=beta, dq_scale=1.0, dz_add=gpu(ste))
    np.testing.assert_allclose(lg.item(), l_vq.item(), rtol=1e-6)
    np.testing.assert_allclose(dz.cpu().numpy(), (gz + ste).numpy(), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(dq.cpu().numpy(), gq.numpy(), rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("N,D,K,dt", [(5120, 128, 512, torch.bfloat16), (3000, 64, 128, torch.bfloat16), (700, 256, 300, torch.bfloat16),
                                      (2048, 128, 64, torch.float32), (130000, 128, 512, torch.bfloat16), (777, 96, 40, torch.bfloat16)])
def test_vq_losses_indexed_with_batchnorm_sums(N, D, K, dt):
    """nsg_vq_losses_indexed_bn: the loss and dz of nsg_vq_losses_indexed bit for bit, plus the backward sums of the BatchNorm whose
    incoming gradient dz is -- against nsg_bn_backward_sums reading the stored dz back (bit for bit for bf16 gradients: the same
    slab walk; 2e-5 of scale for fp32 ones, whose separate pass takes 4 channels per thread), and reproducible."""
    g = torch.Generator().manual_seed(N + D)
    z = gpu(torch.randn(N, D, generator=g))
    e = gpu(torch.randn(K, D, generator=g) * 0.1)
    idx = gpu(torch.randint(0, K, (N,), generator=g))
    add = gpu(torch.randn(N, D, generator=g) * 1e-3).to(dt)
    x = gpu(torch.randn(N, D, generator=g) * 0.5 + 0.2).to(dt)
    mean, invstd = gpu(torch.randn(D, generator=g) * 0.1 + 0.2), gpu(torch.rand(D, generator=g) + 1.0)
    gamma = torch.ones(D, device=DEV)
    assert ops.vq_losses_indexed_bn_supported(D)
    l0, dz0 = ops.vq_losses_indexed(z, e, idx, dz_scale=0.25, dz_add=add, grad_dtype=dt)
    l1, dz1, dg, db = ops.vq_losses_indexed(z, e, idx, dz_scale=0.25, dz_add=add, grad_dtype=dt, bn=(x, mean, invstd))
    assert torch.equal(l0, l1) and torch.equal(dz0, dz1)
    dg_ref, db_ref = ops.bn_backward_sums(x, dz0, mean, invstd, gamma)
    if dt == torch.bfloat16:        # the same slabs in the same order: the separate pass's sums, bit for bit
        assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    _close(dg.cpu(), dg_ref.cpu(), tol=2e-5, what="dgamma")
    _close(db.cpu(), db_ref.cpu(), tol=2e-5, what="dbeta")
    want_b = dz0.double().sum(0)
    want_g = (dz0.double() * ((x.double() - mean.double()) * invstd.double())).sum(0)
    _close(db.double().cpu(), want_b.cpu(), tol=2e-5, what="dbeta vs double")
    _close(dg.double().cpu(), want_g.cpu(), tol=2e-5, what="dgamma vs double")
    _, _, dg2, db2 = ops.vq_losses_indexed(z, e, idx, dz_scale=0.25, dz_add=add, grad_dtype=dt, bn=(x, mean, invstd))
    assert torch.equal(dg, dg2) and torch.equal(db, db2)
    assert ops.vq_losses_indexed_bn_supported(96) and not ops.vq_losses_indexed_bn_supported(100)


def test_adam_matches_torch_optim():
    g = torch.Generator().manual_seed(21)
    p0 = torch.randn(5000, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    pg, m, v = gpu(p0), torch.zeros(5000, device=DEV), torch.zeros(5000, device=DEV)
    for step in range(1, 6):
        grad = torch.randn(5000, generator=g) * (10.0 ** -step)
        ref.grad = grad.clone()
        opt.step()
        ops.adam_step(pg, gpu(grad * 4.0), m, v, step, grad_scale=0.25)
        np.testing.assert_allclose(pg.cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-7)
