"""GPU: the F0-conditioned decoder through the model and the fused training step -- against the CPU autograd oracle of the same
definition (tests/helpers/f0_cond_ref.py), lean against materialised in the bf16 mode, graph replay against the eager step, and
the conversion / training drivers that feed the bins.  Tolerances: test_speaker_conditioned_decoder's and its bf16 companion's
(tests/test_gpu_model.py), the project's own for the same comparison with the speaker table."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import audio, evaluate, models as M, ops, train as T_  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep, vqvae_loss_terms  # noqa: E402
from tests.helpers import f0_cond_ref as R  # noqa: E402

DEV = "cuda:0"
LOSS_RTOL = 1e-5


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def small_case():
    """VQVAE(1, 16, 32, 7 speakers, 8 F0 bins), B = 4, T = 32 (W = 8); speakers 1, 2, 4, 5 and bins 4 and 7 are absent."""
    torch.manual_seed(1)
    model = M.VQVAE(1, 16, 32, n_speakers=7, n_f0_bins=8)
    st0 = {k: v.clone() for k, v in model.state_dict().items()}
    c = torch.rand(4, 1, 80, 32, generator=torch.Generator().manual_seed(7))
    g = torch.tensor([3, 0, 3, 6])
    bins = torch.tensor([[0, 0, 1, 2, 3, 3, 0, 5], [6, 6, 8, 8, 0, 0, 0, 0], [1, 1, 2, 5, 5, 6, 8, 3], [0, 2, 2, 2, 0, 3, 3, 0]])
    return model, st0, c, g, bins


@pytest.fixture(scope="module")
def small_oracle():
    model, st0, c, g, bins = small_case()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return R.conditioned_oracle(st0, c, g, bins)


def test_fused_step_and_autograd_against_the_cpu_oracle(small_oracle):
    model, st0, c, g, bins = small_case()
    lr_, lv, idx, gspk, gf0 = small_oracle
    model = model.to(DEV).train()
    step = FusedTrainStep(model, lr=1e-3)
    # the new slot lies in the back part of the communication buffer, beside the speaker table: the early all-reduce covers it
    lo = step.opt.flat_grad.data_ptr()
    assert step._comm_split > 0
    assert (step.g_f0.data_ptr() - lo) // 4 >= (step.g_spk.data_ptr() - lo) // 4 + step.g_spk.numel() >= step._comm_split
    assert (step.g_f0.data_ptr() - lo) // 4 + step.g_f0.numel() <= step.opt.total
    l = step.forward_backward(c.to(DEV), g.to(DEV), bins.to(DEV))
    assert rel(l[0].item(), lr_.item()) < LOSS_RTOL and rel(l[1].item(), lv.item()) < LOSS_RTOL
    assert int((step.last_indices.cpu() != idx).sum()) == 0
    got_f0, got_spk = model.f0_embedding.weight.grad.cpu(), model.speaker_embedding.weight.grad.cpu()
    np.testing.assert_allclose(got_f0.numpy(), gf0.numpy(), rtol=2e-4, atol=2e-4 * float(gf0.abs().max()))
    np.testing.assert_allclose(got_spk.numpy(), gspk.numpy(), rtol=2e-4, atol=2e-4 * float(gspk.abs().max()))
    assert float(got_f0[[4, 7]].abs().max()) == 0.0 and float(got_f0[[0, 1, 2, 3, 5, 6, 8]].abs().max(1).values.min()) > 0.0     # absent bins
    assert float(got_spk[[1, 2, 4, 5]].abs().max()) == 0.0                                                                       # absent speakers
    # the autograd path gives the same two gradients
    m2 = M.VQVAE(1, 16, 32, n_speakers=7, n_f0_bins=8)
    m2.load_state_dict(st0)
    m2 = m2.to(DEV).train()
    xt, ze, zq = m2(c.to(DEV), g.to(DEV), bins.to(DEV))
    l3 = vqvae_loss_terms(c.to(DEV), xt, ze, zq)
    (l3[0] + l3[1] + l3[2]).backward()
    for a, b in ((m2.f0_embedding.weight.grad, got_f0), (m2.speaker_embedding.weight.grad, got_spk)):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-4, atol=1e-5 * float(b.abs().max()) + 1e-9)
    # a model without the table refuses bins; bins of another shape or type are refused before anything runs
    plain = FusedTrainStep(M.VQVAE(1, 16, 32, n_speakers=7).to(DEV).train(), lr=1e-3)
    with pytest.raises(ValueError, match="without an F0 table"):
        plain.forward_backward(c.to(DEV), g.to(DEV), bins.to(DEV))
    for bad in (bins[:, :7].to(DEV), bins.to(DEV).int(), bins):
        with pytest.raises(ValueError, match="f0_bins must be an int64 tensor of shape"):
            step.forward_backward(c.to(DEV), g.to(DEV), bad)


def test_without_bins_the_step_is_bitwise_the_model_without_the_table():
    model, st0, c, g, bins = small_case()
    model = model.to(DEV).train()
    step = FusedTrainStep(model, lr=1e-3)
    step.forward_backward(c.to(DEV), g.to(DEV), bins.to(DEV))            # leaves a gradient in the F0 slot ...
    assert float(step.g_f0.abs().max()) > 0.0
    model.load_state_dict(st0)                                           # (the BatchNorm running statistics of the start again)
    l = step.forward_backward(c.to(DEV), g.to(DEV))
    assert float(step.g_f0.abs().max()) == 0.0                           # ... which a step without bins zeroes
    plain = M.VQVAE(1, 16, 32, n_speakers=7)
    plain.load_state_dict({k: v for k, v in st0.items() if not k.startswith("f0_embedding")})
    plain = plain.to(DEV).train()
    ps = FusedTrainStep(plain, lr=1e-3)
    lp = ps.forward_backward(c.to(DEV), g.to(DEV))
    assert [x.item() for x in l] == [x.item() for x in lp]
    assert torch.equal(step.last_indices, ps.last_indices)
    ours = dict(model.named_parameters())
    for name, p in plain.named_parameters():
        assert torch.equal(ours[name].grad, p.grad), name
    assert set(ours) - set(dict(plain.named_parameters())) == {"f0_embedding.weight"}


def test_bf16_lean_step_gathers_through_the_indices(monkeypatch):
    """D = 128, K = 512, B = 2, T = 64 (the lean path has no condition on T): with train.LEAN_VQ on, the search writes indices
    alone and one nsg_add_cond call gathers the decoder's bf16 input through them with both rows added; with it off the fp32 z_q is
    materialised and the same entry point adds to its rows."""
    D, K, S, N, B, T = 128, 512, 7, 8, 2, 64
    torch.manual_seed(1)
    model = M.VQVAE(1, D, K, n_speakers=S, n_f0_bins=N, compute_dtype=torch.bfloat16)
    st0 = {k: v.clone() for k, v in model.state_dict().items()}
    c = torch.rand(B, 1, 80, T, generator=torch.Generator().manual_seed(7))
    g = torch.tensor([5, 2])
    bins = torch.randint(0, N + 1, (B, T // 4), generator=torch.Generator().manual_seed(9))
    bins[bins == 4] = 0                                                  # bin 4 is absent
    calls = []
    real = ops.add_cond

    def spy(x, table, bins_, idx=None, **kw):
        y = real(x, table, bins_, idx=idx, **kw)
        calls.append(dict(idx=idx, kw=kw, y=y))
        return y
    monkeypatch.setattr(ops, "add_cond", spy)

    def run(lean):
        monkeypatch.setattr(T_, "LEAN_VQ", lean)
        del calls[:]
        m = M.VQVAE(1, D, K, n_speakers=S, n_f0_bins=N, compute_dtype=torch.bfloat16)
        m.load_state_dict(st0)
        m = m.to(DEV).train()
        st = FusedTrainStep(m, lr=1e-3)
        l = st.forward_backward(c.to(DEV), g.to(DEV), bins.to(DEV))
        return [x_.item() for x_ in l], st.last_indices.clone(), m.f0_embedding.weight.grad.clone(), m.speaker_embedding.weight.grad.clone(), st, list(calls)
    lf, idf, gf, sf, stf, calls_f = run(True)
    lu, idu, gu, su, _, calls_u = run(False)
    assert len(calls_f) == 1 and calls_f[0]["idx"] is not None and calls_f[0]["kw"]["relu"] and calls_f[0]["y"].dtype == torch.bfloat16
    assert len(calls_u) == 1 and calls_u[0]["idx"] is None
    # the lean decoder input, exactly
    cb, spk, f0e = (st0[k].to(DEV) for k in ("codebook.embedding.weight", "speaker_embedding.weight", "f0_embedding.weight"))
    want = torch.relu((cb[idf].view(B, 20, T // 4, D) + spk[g.to(DEV)][:, None, None, :]) + f0e[bins.to(DEV)][:, None, :, :]).to(torch.bfloat16)
    assert torch.equal(calls_f[0]["y"].view(torch.int16), want.view(torch.int16))
    assert torch.equal(idf, idu)
    assert rel(lf[0], lu[0]) < 1e-5 and rel(lf[1], lu[1]) < 1e-5
    assert float((gf - gu).norm() / gu.norm()) < 1e-3 and float((sf - su).norm() / su.norm()) < 1e-3
    assert float(gf[4].abs().max()) == 0.0 and float(sf[0].abs().max()) == 0.0 and float(sf[5].abs().max()) > 0.0
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    lr_, lv, idx_ref, gspk, gf0 = R.conditioned_oracle(st0, c, g, bins)
    assert rel(lf[0], lr_.item()) < 2e-2 and rel(lf[1], lv.item()) < 2e-2
    for name, got, ref in (("F0", gf, gf0), ("speaker", sf, gspk)):
        cos = float(torch.dot(got.cpu().double().flatten(), ref.double().flatten()) / (got.cpu().double().norm() * ref.double().norm()))
        print(f"bf16 lean step: {name}-table gradient cosine vs the fp32 definition {cos:.4f}")
        assert cos > 0.9
    stf.step(c.to(DEV), g.to(DEV), bins.to(DEV))                         # and a full step: Adam moves the table
    assert not torch.equal(stf.model.f0_embedding.weight.detach().cpu(), st0["f0_embedding.weight"])


def test_graph_replay_refills_the_static_bins():
    """Capture with bins, replay with two other bins tensors: losses and the F0 gradient after every step are those of the eager
    step on the same weights and inputs, bit for bit; a step without bins after the capture runs eagerly."""
    _, st0, c, g, bins = small_case()
    c, g = c.to(DEV), g.to(DEV)
    others = [bins.flip(1).contiguous().to(DEV), ((bins + 3) % 9).to(DEV)]
    outs = []
    for use_graph in (False, True):
        m = M.VQVAE(1, 16, 32, n_speakers=7, n_f0_bins=8)
        m.load_state_dict(st0)
        m = m.to(DEV).train()
        st = FusedTrainStep(m, lr=1e-3)
        if use_graph:
            st.capture(c, g, warmup=2, f0_bins=bins.to(DEV))
        else:
            st.step(c, g, bins.to(DEV)); st.step(c, g, bins.to(DEV))
        replays = []
        real = st._replay
        st._replay = lambda *a, **k: (replays.append(1), real(*a, **k))[1]
        rec = []
        for k, b in enumerate(others):
            l = st.step(c * (0.9 - 0.1 * k) + 0.05, g, b)
            rec.append(([x.item() for x in l], m.f0_embedding.weight.grad.clone()))
        assert len(replays) == (2 if use_graph else 0)
        l = st.step(c, g)                                               # no bins: not the captured graph's step
        assert len(replays) == (2 if use_graph else 0) and float(st.g_f0.abs().max()) == 0.0
        outs.append((rec, [x.item() for x in l], {k: v.clone() for k, v in m.state_dict().items()}))
    for (la, ga), (lb, gb) in zip(outs[0][0], outs[1][0]):
        assert la == lb and torch.equal(ga, gb)
    assert not torch.equal(outs[1][0][0][1], outs[1][0][1][1])          # the two replays saw different bins
    assert outs[0][1] == outs[1][1]
    for k in outs[0][2]:
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k


def test_convert_voice_decodes_under_the_bins():
    model, st0, c, g, bins = small_case()
    model = model.to(DEV).train()
    mel = c.to(DEV)
    codes, mels = evaluate.convert_voice(model, mel, g, bins.to(DEV))
    assert model.training and tuple(codes.shape) == (4, 20, 8) and tuple(mels.shape) == (4, 1, 80, 32)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.encode(mel), codes)
        assert torch.equal(model.decode(codes, g.to(DEV), bins.to(DEV)), mels)
        assert not torch.equal(model.decode(codes, g.to(DEV)), mels)                      # None adds no F0 term
    _, other = evaluate.convert_voice(model, mel, g, ((bins + 3) % 9).to(DEV))
    assert not torch.equal(other, mels)
    _, host = evaluate.convert_voice(model, mel, g, bins)                                 # bins on the host are moved
    assert torch.equal(host, mels)


def test_train_conditioned_feeds_the_tracked_bins(tmp_path):
    from neural_sound_generation_amd import data as Dm
    root = str(tmp_path / "arctic")
    Dm.write_synthetic_data_root(root, n_utts=7, min_frames=40, max_frames=60, n_speakers=2, with_audio=True, seed=5)
    loaders = Dm.get_data_loaders(root, batch_size=2, num_workers=0, with_audio=True, frame_multiple=4, pin_memory=False)

    class Fixed:                                                         # the epoch's batches, kept so they can be tracked again
        dataset = loaders["train"].dataset
        batches = list(loaders["train"])

        def __iter__(self):
            return iter(self.batches)
    assert 2 <= len(Fixed.batches) <= 3
    torch.manual_seed(1)
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).to(DEV)
    before = model.f0_embedding.weight.detach().clone()
    step = FusedTrainStep(model, lr=1e-3)
    fed = []
    real = step.step
    step.step = lambda c, g=None, f0_bins=None: (fed.append((c, g, f0_bins)), real(c, g, f0_bins=f0_bins))[1]

    class A:
        log_interval = 1
    loss = T_.train_conditioned(A(), model, step, Fixed(), DEV, 0)
    assert np.isfinite(loss) and len(fed) == len(Fixed.batches) and model.training
    assert not torch.equal(model.f0_embedding.weight.detach(), before)
    for (x, y, c, g, lens), (c_fed, g_fed, bins) in zip(Fixed.batches, fed):
        T = c.shape[2]
        B = len(c)
        assert x is not None and tuple(x.shape) == (B, 1, T * 256) and torch.equal(c_fed.cpu(), c.unsqueeze(1)) and torch.equal(g_fed.cpu(), g)
        f0, _ = audio.f0(x.squeeze(1).to(DEV).contiguous(), lengths=lens.numpy())
        assert f0.shape[1] == T + 1
        want = audio.f0_bins(f0[:, :T // 4 * 4].contiguous(), frames=lens.numpy() // 256, n_bins=8, fmin=65.0, fmax=500.0)
        assert tuple(bins.shape) == (B, T // 4) and torch.equal(bins, want)
    # a loader without audio cannot feed an F0-conditioned model
    mel_only = Dm.get_data_loaders(root, batch_size=2, num_workers=0, frame_multiple=4, pin_memory=False)
    with pytest.raises(ValueError, match=r"get_data_loaders\(with_audio=True\)"):
        T_.train_conditioned(A(), model, step, mel_only["train"], DEV, 0)


def test_test_conversion_f0_moves_the_contour_to_the_target_statistics(monkeypatch):
    import tests.test_gpu_f0_stats as S                                  # its pair_batch: gliding harmonic tones with a quiet tail
    torch.manual_seed(13)
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).to(DEV).train()
    loader = [S.pair_batch(1, 10240, 11000), S.pair_batch(2, 9000, 8200)]
    stats = np.array([[np.log2(170.0), 0.09], [np.log2(210.0), 0.06]])
    seen = []
    real = evaluate.convert_voice

    def spy(vqvae, mel, g_target, f0_bins=None):
        seen.append((g_target, f0_bins))
        return real(vqvae, mel, g_target, f0_bins)
    monkeypatch.setattr(evaluate, "convert_voice", spy)
    gen = torch.Generator().manual_seed(4)
    angles = [torch.rand(2, (1 + b[0].shape[1] // 256) // 4 * 4, 513, generator=gen).to(DEV) for b in loader]
    got = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, angles0=angles, f0_stats=stats)
    assert got["clips"] == 4 and len(seen) == 2 and model.training
    for side in ("converted", "source"):
        assert all(np.isfinite(got[side][k]) for k in ("vuv_error", "mcd")) and np.isfinite(got[side]["stats"]).all()
    assert np.isfinite(got["converted"]["spectral_convergence"]) and np.isfinite(got["source"]["f0_rmse_cents"])
    voiced_columns = 0
    for (ws, ls, wt, lt, g), (g_seen, bins) in zip(loader, seen):
        assert torch.equal(g_seen, g) and bins is not None and bins.dtype == torch.int64
        f0_s, _ = audio.f0(ws.to(DEV), lengths=ls)
        Tc = f0_s.shape[1] // 4 * 4
        fc = np.minimum(1 + ls.numpy() // 256, Tc) // 4 * 4
        f = f0_s[:, :Tc].cpu().numpy()
        affine = R.affine_f64(R.logf0_sums_f64(f, fc), stats[g.numpy(), 0], stats[g.numpy(), 1])
        b64, _, u64, voiced = R.bins_f64(f, Tc // 4, 8, 65.0, 500.0, fc, affine)
        dec = R.decided(u64)
        got_b = bins.cpu().numpy()
        assert got_b.shape == b64.shape and np.array_equal(got_b[dec | ~voiced], b64[dec | ~voiced])
        assert np.abs(got_b - b64).max() <= 1
        voiced_columns += int(voiced.sum())
        # the move did something: the bins differ from those of the unmoved contour
        assert not np.array_equal(b64, R.bins_f64(f, Tc // 4, 8, 65.0, 500.0, fc)[0])
    assert voiced_columns >= 20
    # without statistics the contour is the source's own
    del seen[:]
    evaluate.test_conversion_f0(None, model, loader[:1], DEV, 0, iters=2, angles0=angles[:1])
    ws, ls = loader[0][0], loader[0][1]
    f0_s, _ = audio.f0(ws.to(DEV), lengths=ls)
    fc = np.minimum(1 + ls.numpy() // 256, 40) // 4 * 4
    assert torch.equal(seen[0][1], audio.f0_bins(f0_s[:, :40].contiguous(), frames=fc, n_bins=8))
