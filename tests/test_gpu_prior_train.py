"""GPU: stage two of the model family -- the masked cross-entropy with per-clip sums, the gate of a sum with fused column
sums, PriorTrainStep against the autograd path, the reference fixture and the fp64 oracle, and the loops from a data root.

Reference of the masked loss: the reference project never trains this model, so there is no fixture for it (parity
unpinned); it is pinned by fp64 F.cross_entropy(..., ignore_index=-1) on the oracle's logits (oracle/pixelcnn_oracle.py) with
the model of tests/golden/prior_tiny.npz, and kernel by kernel by fp64 torch on the same fp32 inputs."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import ops  # noqa: E402
from neural_sound_generation_amd.optim import FlatAdam  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from neural_sound_generation_amd.prior_train import PriorTrainStep  # noqa: E402
from oracle import pixelcnn_oracle as P  # noqa: E402
from tests.test_gpu_prior import build  # noqa: E402
from tests.test_gpu_prior_width import _ce64, _ce_logits  # noqa: E402

DEV = "cuda:0"


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---------------------------------------------------------------------------------------------
# 1a. masked cross-entropy
# ---------------------------------------------------------------------------------------------
CE_GRIDS = {1: (1, 1, 1), 7: (1, 1, 7), 4096: (4, 4, 256), 327680: (64, 20, 256)}        # M -> (B, H, W)
CE_FAMILIES = ["randn", "offset+200", "confident", "tied", "constant"]
CE_MASKS = ["none", "ragged", "one_clip", "all"]


def _mask(kind, B, H, W, gen):
    """bool (B, H, W): the valid positions."""
    if kind == "none":
        lengths = torch.full((B,), W, device=DEV)
    elif kind == "ragged":
        lengths = torch.randint(0, W + 1, (B,), device=DEV, generator=gen)
        if B > 1:
            lengths[0], lengths[-1] = W, max(W // 3, 1)          # (at least one full and one partial clip)
    elif kind == "one_clip":
        lengths = torch.full((B,), W, device=DEV)
        lengths[0] = 0
    else:
        lengths = torch.zeros(B, dtype=torch.int64, device=DEV)
    return (torch.arange(W, device=DEV)[None, None, :] < lengths[:, None, None]).expand(B, H, W)


@pytest.mark.parametrize("family", CE_FAMILIES)
def test_masked_cross_entropy_against_fp64(family):
    gen = torch.Generator(device=DEV).manual_seed(11 + CE_FAMILIES.index(family))
    for M, (B, H, W) in CE_GRIDS.items():
        for K in (32, 512):
            l, t_full = _ce_logits(family, M, K, gen)
            for kind in CE_MASKS:
                for gs in (1.0, 0.37):
                    what = f"{family} M={M} K={K} mask={kind} grad_scale={gs}"
                    valid = _mask(kind, B, H, W, gen).reshape(-1)
                    t = torch.where(valid, t_full, torch.full_like(t_full, -1))
                    loss, dl, nll, cnt = ops.cross_entropy_masked(l, t, H * W, grad_scale=gs, want_clip=True)
                    n_valid = int(valid.sum())
                    assert torch.equal(cnt, valid.view(B, -1).sum(1)), what                       # clip_count exact
                    assert bool((dl[~valid] == 0).all()), f"{what}: an ignored row has a non-zero gradient"
                    if n_valid == 0:
                        assert float(loss) == 0.0 and bool((dl == 0).all()) and bool((nll == 0).all()), what
                        continue
                    want, g64 = _ce64(l[valid], t[valid], gs)          # fp64 on the valid rows: their mean, gradient * gs / n_valid
                    got = float(loss)
                    print(f"{what}: loss {got!r} fp64 {float(want)!r} rel {rel(got, float(want)):.2e}")
                    assert rel(got, float(want)) <= 1e-6, what
                    err = (dl[valid].double() - g64).abs().amax(dim=1)
                    bound = 1e-5 * g64.abs().amax(dim=1)
                    assert not bool((err > bound).any()), f"{what}: {int((err > bound).sum())} valid rows' gradients beyond 1e-5 of the row scale"
                    ratio = float(nll.double().sum()) / float(cnt.sum())
                    assert rel(ratio, got) <= 1e-6, f"{what}: sum clip_nll / sum clip_count {ratio!r} vs loss {got!r}"
                    if kind == "none":                                  # nothing ignored: the unmasked kernel's results, bit for bit
                        l0, d0 = ops.cross_entropy(l, t_full, grad_scale=gs)
                        assert torch.equal(l0, loss) and torch.equal(d0, dl), what
                    if gs == 1.0:
                        l2, d2, n2, c2 = ops.cross_entropy_masked(l, t, H * W, grad_scale=gs, want_clip=True)        # two runs, identical bits
                        assert torch.equal(l2, loss) and torch.equal(d2, dl) and torch.equal(n2, nll) and torch.equal(c2, cnt), what
                        for b in sorted({0, B - 1}):                    # a clip's sum from its rows alone
                            rows = slice(b * H * W, (b + 1) * H * W)
                            _, _, n1, c1 = ops.cross_entropy_masked(l[rows].contiguous(), t[rows].contiguous(), H * W, want_grad=False, want_clip=True)
                            assert int(c1) == int(cnt[b]), what
                            assert abs(float(n1) - float(nll[b])) <= 1e-6 * abs(float(nll[b])), f"{what}: clip {b} alone {float(n1)!r} vs in the batch {float(nll[b])!r}"


def test_masked_cross_entropy_ignores_targets_past_k():
    """A target >= K violates the precondition; the row is treated as ignored (and never read out of range)."""
    gen = torch.Generator(device=DEV).manual_seed(3)
    l = torch.randn(24, 32, device=DEV, generator=gen)
    t = torch.randint(0, 32, (24,), device=DEV, generator=gen)
    t[5], t[17] = 32, 1 << 40
    loss, dl, nll, cnt = ops.cross_entropy_masked(l, t, 12, want_clip=True)
    keep = t < 32
    want, g64 = _ce64(l[keep], t[keep], 1.0)
    assert rel(float(loss), float(want)) <= 1e-6 and cnt.tolist() == [11, 11] and bool((dl[~keep] == 0).all())


# ---------------------------------------------------------------------------------------------
# 1b / 1c. the gate of a sum, the fused column sums
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(3, 5, 7, 12), (4, 20, 64, 64), (2, 3, 5, 256), (1, 1, 1, 4)])
@pytest.mark.parametrize("scale", [1.0, 20.0], ids=["unit", "saturated"])
def test_gate_of_a_sum_and_fused_column_sums(B, H, W, C, scale):
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + C)
    a = torch.randn(B, H, W, 2 * C, device=DEV, generator=gen) * scale           # saturated: |a + b| reaches 40 and beyond
    b = torch.randn(B, H, W, 2 * C, device=DEV, generator=gen) * scale
    cond = torch.randn(B, 2 * C, device=DEV, generator=gen)
    dy = torch.randn(B, H, W, C, device=DEV, generator=gen)
    if scale > 1:
        a.view(-1)[:2] = torch.tensor([30.0, -30.0], device=DEV)
        b.view(-1)[:2] = torch.tensor([10.0, -10.0], device=DEV)
        assert float((a + b).abs().max()) >= 40
    s = ops.add(a, b)
    for cd in (cond, None):
        what = f"{(B, H, W, C)} cond={'yes' if cd is not None else 'no'}"
        y = ops.gated_activation_sum(a, b, cd)
        assert torch.equal(y, ops.gated_activation(s, cd)) and bool(torch.isfinite(y).all()), what
        want_dx = ops.gated_activation_backward(s, cd, dy)
        dx, none = ops.gated_activation_sum_backward(a, b, cd, dy)
        assert none is None and torch.equal(dx, want_dx) and bool(torch.isfinite(dx).all()), what
        # the column sums, fused: sum form and plain form
        dx1, dc1 = ops.gated_activation_sum_backward(a, b, cd, dy, want_dcond=True, n_clips=B)
        dx2, dc2 = ops.gated_activation_backward_colsum(s, cd, dy, n_clips=B)
        assert torch.equal(dx1, want_dx) and torch.equal(dx2, want_dx) and torch.equal(dc1, dc2), what
        ref32 = ops.clip_colsum(want_dx, B).cpu().numpy()
        ref64 = want_dx.double().view(B, -1, 2 * C).sum(1).cpu().numpy()
        np.testing.assert_allclose(dc1.cpu().numpy(), ref32, rtol=1e-4, atol=1e-5, err_msg=what)
        np.testing.assert_allclose(dc1.cpu().numpy(), ref64, rtol=1e-4, atol=1e-5, err_msg=what)
        _, dc3 = ops.gated_activation_sum_backward(a, b, cd, dy, want_dcond=True, n_clips=B)
        assert torch.equal(dc3, dc1), what                                        # two runs, identical bits
    if scale > 1:
        return
    # against fp64 autograd: y and both gradients
    a64, b64, c64 = (v.double().requires_grad_(True) for v in (a, b, cond))
    u, v = ((a64 + b64) + c64[:, None, None, :]).chunk(2, dim=-1)
    y64 = torch.tanh(u) * torch.sigmoid(v)
    ga, gc = torch.autograd.grad(y64, [a64, c64], dy.double())
    np.testing.assert_allclose(ops.gated_activation_sum(a, b, cond).cpu().numpy(), y64.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    dx, dc = ops.gated_activation_sum_backward(a, b, cond, dy, want_dcond=True)
    np.testing.assert_allclose(dx.cpu().numpy(), ga.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dc.cpu().numpy(), gc.cpu().numpy(), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# 2. the fused step against the autograd step, the reference fixture and the fp64 oracle
# ---------------------------------------------------------------------------------------------
def _ragged_batch(input_dim=32, n_classes=4):
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, input_dim, (3, 20, 12), generator=gen)
    label = torch.randint(0, n_classes, (3,), generator=gen)
    return x, label, torch.tensor([12, 7, 0])


def _both_paths(make, x, label, lengths, lr=1e-3):
    """(autograd loss, its FlatAdam, its model), (fused loss, the step): the same model twice, gradients in the flat buckets."""
    ma = make()
    oa = FlatAdam(ma.parameters(), lr=lr)
    oa.zero_grad()
    la = ma.loss(x.to(DEV), label.to(DEV)) if lengths is None else ma.loss(x.to(DEV), label.to(DEV), lengths.to(DEV))
    la.backward()
    step = PriorTrainStep(make(), lr=lr)
    lf = step.forward_backward(x.to(DEV), label.to(DEV), None if lengths is None else lengths.to(DEV))
    return (la, oa, ma), (lf, step)


def _assert_flat_grads(step, oa, what):
    ga, gf = oa.flat_grad.cpu().numpy(), step.opt.flat_grad.cpu().numpy()
    scale = float(np.abs(ga).max())
    print(f"{what}: max|g| {scale:.3e}, max |fused - autograd| {float(np.abs(gf - ga).max()):.3e}")
    np.testing.assert_allclose(gf, ga, rtol=1e-5, atol=1e-7 * scale, err_msg=what)
    for p in step.model.parameters():                      # every p.grad is a view of the bucket
        lo = p.grad.data_ptr() - step.opt.flat_grad.data_ptr()
        assert 0 <= lo < 4 * step.opt.flat_grad.numel()


@pytest.mark.parametrize("case", ["fixture", "ragged"])
def test_fused_step_equals_autograd_step(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "prior_tiny.npz"))
    n_layers = int(g["cfg"][2])
    if case == "fixture":
        x, label, lengths = torch.from_numpy(g["x"]), torch.from_numpy(g["label"]), None
    else:
        x, label, lengths = _ragged_batch(int(g["cfg"][0]), int(g["cfg"][3]))
    (la, oa, ma), (lf, step) = _both_paths(lambda: build(g)[0], x, label, lengths)
    print(f"{case}: fused loss {lf.item()!r} autograd {la.item()!r}")
    assert rel(lf.item(), la.item()) < 1e-6
    _assert_flat_grads(step, oa, case)
    # against the reference fixture (no mask) / the fp64 oracle with ignore_index (mask)
    if lengths is None:
        want_loss = float(g["loss"])
        want_grads = {k: g["grad." + k] for k, _ in step.model.named_parameters()}
    else:
        st = {k[4:]: torch.from_numpy(np.array(g[k])).double() for k in g.files if k.startswith("sd0.")}
        params = {k: v.clone().requires_grad_(True) for k, v in st.items()}
        target = torch.where(torch.arange(x.shape[2])[None, None, :] < lengths[:, None, None], x, torch.full_like(x, -1))
        loss64 = F.cross_entropy(P.forward(params, x, label, n_layers), target, ignore_index=-1)
        grads = torch.autograd.grad(loss64, list(params.values()))
        want_loss, want_grads = float(loss64.detach()), {k: v.numpy() for k, v in zip(params, grads)}
    assert rel(lf.item(), want_loss) <= 1e-5
    for k, p in step.model.named_parameters():
        w = want_grads[k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), w, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(w).max())), err_msg=k)
    # one Adam step on both (a step moves a parameter by at most lr), then layer 0's masked taps are zero again after a forward
    oa.step()
    step.opt.step()
    np.testing.assert_allclose(step.opt.flat_param.cpu().numpy(), oa.flat_param.cpu().numpy(), rtol=0, atol=2.1e-3)
    l0 = step.model.layers[0]
    assert float(l0.vert_stack.weight.detach()[:, :, -1].abs().max()) > 0          # Adam moved them (their gradients are the kernel's, non-zero)
    step.forward_backward(x.to(DEV), label.to(DEV), None if lengths is None else lengths.to(DEV))
    assert bool((l0.vert_stack.weight[:, :, -1] == 0).all()) and bool((l0.horiz_stack.weight[:, :, :, -1] == 0).all())


def test_all_clips_too_short_gives_zero_loss_and_gradient(golden_dir):
    g = np.load(os.path.join(golden_dir, "prior_tiny.npz"))
    x, label, _ = _ragged_batch(int(g["cfg"][0]), int(g["cfg"][3]))
    step = PriorTrainStep(build(g)[0])
    step.opt.flat_grad.fill_(7.0)
    loss = step.forward_backward(x.to(DEV), label.to(DEV), torch.zeros(3, dtype=torch.int64))
    assert float(loss) == 0.0
    for k, p in step.model.named_parameters():
        assert bool((p.grad == 0).all()), k


def test_fused_steps_train(golden_dir):
    """Ten fused steps at lr 3e-3 on a fixed ragged batch end below the first loss (fp64 oracle + torch Adam on the same model
    and batch: 3.4877 -> 2.6637); the autograd path + FlatAdam follows the same trajectory; two fused runs give identical bits."""
    g = np.load(os.path.join(golden_dir, "prior_tiny.npz"))
    x, label, lengths = (v.to(DEV) for v in _ragged_batch(int(g["cfg"][0]), int(g["cfg"][3])))
    runs = []
    for _ in range(2):
        step = PriorTrainStep(build(g)[0], lr=3e-3)
        losses = [step.step(x, label, lengths).item() for _ in range(10)]
        runs.append((losses, step.opt.flat_param.clone()))
    print("fused trajectory:", runs[0][0])
    assert runs[0][0][-1] < runs[0][0][0]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    ma = build(g)[0]
    oa = FlatAdam(ma.parameters(), lr=3e-3)
    auto = []
    for _ in range(5):
        oa.zero_grad()
        l = ma.loss(x, label, lengths)
        l.backward()
        oa.step()
        auto.append(l.item())
    np.testing.assert_allclose(runs[0][0][:5], auto, rtol=5e-4)


def test_production_width():
    torch.manual_seed(2)
    proto = GatedPixelCNN(512, 64, 15)
    sd = {k: v.clone() for k, v in proto.state_dict().items()}

    def make():
        m = GatedPixelCNN(512, 64, 15)
        m.load_state_dict(sd)
        return m.to(DEV)
    gen = torch.Generator().manual_seed(9)
    x = torch.randint(0, 512, (4, 20, 256), generator=gen)
    label = torch.randint(0, 10, (4,), generator=gen)
    lengths = torch.tensor([256, 131, 0, 17])
    (la, oa, ma), (lf, step) = _both_paths(make, x, label, lengths)
    print(f"production width: fused loss {lf.item()!r} autograd {la.item()!r}")
    assert rel(lf.item(), la.item()) < 1e-6
    _assert_flat_grads(step, oa, "production width 4x20x256")
    del oa, ma, la
    torch.cuda.empty_cache()
    x = torch.randint(0, 512, (64, 20, 256), generator=gen)
    label = torch.randint(0, 10, (64,), generator=gen)
    loss = step.step(x.to(DEV), label.to(DEV), torch.randint(0, 257, (64,), generator=gen))
    assert np.isfinite(loss.item()) and loss.item() > 0


# ---------------------------------------------------------------------------------------------
# 3. from a data root: codes_from_mels, train_prior / test_prior, run_prior_epoch, checkpoints, sampling
# ---------------------------------------------------------------------------------------------
class _Args:
    model, dataset, dim, z_dim, beta, log_interval = "pixelcnn", "arctic", 16, 32, 1.0, 1000

    def __init__(self, sampledir):
        self.sampledir = sampledir


def test_prior_from_a_data_root(tmp_path, monkeypatch):
    from neural_sound_generation_amd import data as Dm, evaluate as E, models as M
    from neural_sound_generation_amd.epoch import run_prior_epoch
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / "arctic")
    Dm.write_synthetic_data_root(root, n_utts=12, n_speakers=3, with_audio=False, seed=3)
    loaders = Dm.get_data_loaders(root, batch_size=4, num_workers=0, frame_multiple=4, test_size=0.25)
    torch.manual_seed(1)
    vqvae = M.VQVAE(1, 16, 32).to(DEV).train()
    before = {k: v.clone() for k, v in vqvae.state_dict().items()}

    # codes and lengths of every batch
    for x, y, c, g, input_lengths in loaders["test"]:
        codes, lengths = E.codes_from_mels(vqvae, c.to(DEV).unsqueeze(1), input_lengths)
        frames = (c.abs().sum(1) > 0).sum(1)                                  # the clip's own frames: the rest is zero padding
        assert codes.dtype == torch.int64 and tuple(codes.shape) == (len(c), 20, c.shape[2] // 4)
        assert lengths.dtype == torch.int64 and torch.equal(lengths.cpu(), frames // 4) and int(lengths.max()) == codes.shape[2]
        assert int(codes.min()) >= 0 and int(codes.max()) < 32 and g is not None
    assert vqvae.training
    for k, v in vqvae.state_dict().items():
        assert torch.equal(v, before[k]), k

    def fresh():
        torch.manual_seed(4)
        prior = GatedPixelCNN(32, 16, 3, 3).to(DEV)
        return prior, PriorTrainStep(prior, lr=3e-3)

    def epoch(prior, step, n, **kw):
        random.seed(100 + n)
        np.random.seed(100 + n)
        return run_prior_epoch(_Args(str(tmp_path / "samples")), vqvae, prior, step, loaders["train"], loaders["test"], DEV, n,
                               checkpoint_path=str(tmp_path / f"prior_{n}.pth.tar"), **kw)

    prior, step = fresh()
    r1, r2 = epoch(prior, step, 1), epoch(prior, step, 2)
    for r in (r1, r2):
        assert np.isfinite(r["train_loss"]) and np.isfinite(r["test_nats_per_code"]) and r["test_nats_per_code"] > 0
    for k, v in vqvae.state_dict().items():                                   # the VQ-VAE is never updated
        assert torch.equal(v, before[k]), k

    # test_prior = sum nll / sum count over the same batches
    nll, cnt = 0.0, 0
    for x, y, c, g, input_lengths in loaders["test"]:
        codes, lengths = E.codes_from_mels(vqvae, c.to(DEV).unsqueeze(1), input_lengths)
        a, b = prior.nll(codes, g, lengths)
        assert torch.equal(b.cpu(), 20 * lengths.cpu())
        nll, cnt = nll + float(a.double().sum()), cnt + int(b.sum())
    got = E.test_prior(_Args(""), vqvae, prior, loaders["test"], DEV, 2)
    assert rel(got, nll / cnt) <= 1e-6 and rel(got, r2["test_nats_per_code"]) <= 1e-6

    # resume from the checkpoint of epoch 2: epoch 3 equals the uninterrupted one bit for bit
    r3 = epoch(prior, step, 3)
    prior_b, step_b = fresh()
    st = E.load_checkpoint(r2["checkpoint"], prior_b, step_b.opt, map_location=DEV)
    assert st["epoch"] == 2 and st["arch"] == "pixelcnn"
    r3b = epoch(prior_b, step_b, 3)
    assert r3b["train_loss"] == r3["train_loss"] and r3b["test_nats_per_code"] == r3["test_nats_per_code"]
    assert torch.equal(step_b.opt.flat_param, step.opt.flat_param) and torch.equal(step_b.opt.exp_avg_sq, step.opt.exp_avg_sq)

    # samples of the trained prior
    r4 = epoch(prior, step, 4, sample_label=torch.tensor([0, 2]), sample_frames=32)
    codes = r4["sample_codes"]
    assert tuple(codes.shape) == (2, 20, 8) and codes.dtype == torch.int64 and int(codes.min()) >= 0 and int(codes.max()) < 32
    mels = np.load(r4["samples"], allow_pickle=False)
    assert mels.shape == (2, 80, 32) and mels.dtype == np.float32 and np.isfinite(mels).all()

    # the autograd form of the loop (a torch optimiser) runs on the same loader
    prior_c, _ = fresh()
    from neural_sound_generation_amd.prior_train import train_prior
    random.seed(101)
    la = train_prior(_Args(""), vqvae, prior_c, torch.optim.Adam(prior_c.parameters(), lr=3e-3), loaders["train"], DEV, 1)
    assert rel(la, r1["train_loss"]) <= 5e-4

    # clips of one length: no padding, so the test figure does not depend on the batch size
    root2 = str(tmp_path / "even")
    Dm.write_synthetic_data_root(root2, n_utts=12, min_frames=64, max_frames=64, n_speakers=3, with_audio=False, seed=7)
    figs = [E.test_prior(_Args(""), vqvae, prior, Dm.get_data_loaders(root2, batch_size=bs, num_workers=0, frame_multiple=4, test_size=0.5)["test"], DEV, 0)
            for bs in (1, 4, 12)]
    print("test_prior at batch sizes 1, 4, 12:", figs)
    assert rel(figs[1], figs[0]) <= 1e-6 and rel(figs[2], figs[0]) <= 1e-6
