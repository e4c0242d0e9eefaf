"""GPU: the pitch perturbation above the kernels -- FusedTrainStep's `target` (the reconstruction loss against another mel than
the encoder's input) against the step without it and against the autograd path, eager and under a captured graph;
train.train_conditioned(pitch_perturb=); evaluate.test_conversion_f0(psola_baseline=).  Tolerances for fused against autograd are
tests/test_gpu_model.py's: test_tiny_model_fused_step_equals_autograd_step's in fp32, test_bf16_mode_against_fp32_oracle's
in bf16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import data as Dm, evaluate, models as M, train as T_  # noqa: E402
from neural_sound_generation_amd.optim import FlatAdam  # noqa: E402
from neural_sound_generation_amd.train import FusedTrainStep, vqvae_loss_terms  # noqa: E402
import tests.test_gpu_model as GM  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


def tiny(golden_dir, dtype):
    """tests/golden/model_tiny.npz's model in `dtype` mode and its first batch, with a second mel of the same shape."""
    g = GM.golden(golden_dir, "model_tiny.npz")
    dim, z_dim = (int(v) for v in g["cfg"])
    model = M.VQVAE(1, dim, z_dim, compute_dtype=dtype) if dtype != torch.float32 else M.VQVAE(1, dim, z_dim)
    model.load_state_dict({k[4:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd0.")})
    c = torch.from_numpy(g["s0.c"]).to(DEV)
    c2 = (c.flip(3) * 0.9 + 0.05).contiguous()
    return model.to(DEV).train(), c, c2


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_target_equal_to_the_input_is_the_step_bit_for_bit(golden_dir, dtype):
    outs = []
    for with_target in (False, True):
        model, c, _ = tiny(golden_dir, dtype)
        step = FusedTrainStep(model, lr=1e-3)
        l = step.step(c, target=c.clone()) if with_target else step.step(c)
        outs.append(([x.item() for x in l], step.opt.flat_grad.clone(), step.opt.flat_param.clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    with pytest.raises(ValueError, match="target must be a float32 tensor of c's shape"):
        step.step(c, target=c[:, :, :, :-4].contiguous())
    with pytest.raises(ValueError, match="target must be a float32 tensor of c's shape"):
        step.step(c, target=c.cpu())
    with pytest.raises(ValueError, match="target must be a float32 tensor of c's shape"):
        step.step(c, target=c.double())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_loss_and_the_decoder_gradients_follow_the_target(golden_dir, dtype):
    ma, c, c2 = tiny(golden_dir, dtype)
    oa = FlatAdam(ma.parameters(), lr=1e-3)
    oa.zero_grad()
    xt, ze, zq = ma(c2)
    l3 = vqvae_loss_terms(c, xt, ze, zq)                                 # mse(x_tilde(c2), c): the encoder saw c2, the loss compares with c
    (l3[0] + l3[1] + l3[2]).backward()
    mf, _, _ = tiny(golden_dir, dtype)
    step = FusedTrainStep(mf, lr=1e-3, beta=1.0)
    lf = step.forward_backward(c2, target=c)
    own = FusedTrainStep(tiny(golden_dir, dtype)[0], lr=1e-3, beta=1.0).forward_backward(c2)
    assert GM.rel(own[0].item(), lf[0].item()) > 1e-3                    # the target is not the input: another loss
    loss_rtol = 1e-6 if dtype == torch.float32 else 1e-5
    assert GM.rel(lf[0].item(), l3[0].item()) < loss_rtol and GM.rel(lf[1].item(), l3[1].item()) < loss_rtol
    checked = 0
    for (k, p), (_, q) in zip(mf.named_parameters(), ma.named_parameters()):
        if not k.startswith("decoder.") or GM.is_noise_bias(k):
            continue
        if dtype == torch.float32:
            ga = q.grad.cpu().numpy()
            np.testing.assert_allclose(p.grad.cpu().numpy(), ga, rtol=1e-5, atol=1e-7 * max(1.0, np.abs(ga).max()), err_msg=k)
        else:
            assert torch.allclose(p.grad, q.grad, rtol=1e-4, atol=1e-6 * float(p.grad.abs().max()) + 1e-12), k
        checked += 1
    assert checked >= 8


def test_a_graph_captured_without_a_target_is_not_replayed_for_a_step_with_one(golden_dir):
    outs = []
    for use_graph in (False, True):
        model, c, c2 = tiny(golden_dir, torch.float32)
        st = FusedTrainStep(model, lr=1e-3)
        if use_graph:
            st.capture(c, warmup=2)
        else:
            st.step(c); st.step(c)
        replays = []
        real = st._replay
        st._replay = lambda *a, **k: (replays.append(1), real(*a, **k))[1]
        la = [x.item() for x in st.step(c2)]                             # without a target: the captured step
        assert len(replays) == (1 if use_graph else 0)
        lb = [x.item() for x in st.step(c2, target=c)]                   # with one: eager, whatever was captured
        assert len(replays) == (1 if use_graph else 0)
        outs.append((la, lb, st.opt.flat_grad.clone(), st.opt.flat_param.clone()))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][0] != outs[0][1]
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])


def test_a_graph_captured_with_a_target_refills_it(golden_dir):
    outs = []
    for use_graph in (False, True):
        model, c, c2 = tiny(golden_dir, torch.float32)
        st = FusedTrainStep(model, lr=1e-3)
        if use_graph:
            st.capture(c2, warmup=2, target=c)
        else:
            st.step(c2, target=c); st.step(c2, target=c)
        replays = []
        real = st._replay
        st._replay = lambda *a, **k: (replays.append(1), real(*a, **k))[1]
        la = [x.item() for x in st.step(c2, target=(c * 0.5).contiguous())]      # (a replay's losses live in the graph's own tensors: read now)
        lb = [x.item() for x in st.step(c, target=c2)]
        assert len(replays) == (2 if use_graph else 0) and la != lb
        lc = [x.item() for x in st.step(c2)]                             # no target: not this graph's step
        assert len(replays) == (2 if use_graph else 0)
        outs.append((la + lb + lc, st.opt.flat_param.clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])


class Args:
    log_interval = 100


def test_train_conditioned_with_pitch_perturbation(tmp_path):
    root = str(tmp_path / "voiced")
    Dm.write_synthetic_data_root(root, n_utts=7, min_frames=40, max_frames=60, n_speakers=2, with_audio=True, seed=5, voiced=True)
    loaders = Dm.get_data_loaders(root, batch_size=2, num_workers=0, with_audio=True, frame_multiple=4, pin_memory=False)

    class Fixed:
        dataset = loaders["train"].dataset
        batches = list(loaders["train"])

        def __iter__(self):
            return iter(self.batches)

    def epoch(perturb, seed=None, spy=None):
        torch.manual_seed(1)
        model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).to(DEV)
        step = FusedTrainStep(model, lr=1e-3)
        if spy is not None:
            real = step.step
            step.step = lambda c, g=None, f0_bins=None, target=None: (spy.append((c, f0_bins, target)), real(c, g, f0_bins=f0_bins, target=target))[1]
        kw = {} if perturb is None else dict(pitch_perturb=perturb, generator=torch.Generator().manual_seed(seed))
        loss = T_.train_conditioned(Args(), model, step, Fixed(), DEV, 0, **kw)
        assert np.isfinite(loss) and model.training
        return step.opt.flat_param.clone()
    fed = []
    a, b, other, plain = epoch((-3.0, 3.0), 11, fed), epoch((-3.0, 3.0), 11), epoch((-3.0, 3.0), 12), epoch(None)
    assert torch.equal(a, b) and not torch.equal(a, other) and not torch.equal(a, plain)
    assert len(fed) == len(Fixed.batches) >= 2
    for (x, y, c, g, lens), (c_in, bins, target) in zip(Fixed.batches, fed):
        assert torch.equal(target.cpu(), c.unsqueeze(1)) and c_in.shape == target.shape and not torch.equal(c_in, target)      # the loss target is the clean mel
        assert bins is not None and tuple(bins.shape) == (len(c), c.shape[2] // 4)
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).to(DEV)
    step = FusedTrainStep(model, lr=1e-3)
    before = step.opt.flat_param.clone()
    x, y, c, g, lens = Fixed.batches[0]
    resident = (None, None, c, g, lens, torch.zeros(len(c), c.shape[2] // 4, dtype=torch.int64))       # a resident loader's six-tuple: no audio
    mel_only = Dm.get_data_loaders(root, batch_size=2, num_workers=0, frame_multiple=4, pin_memory=False)["train"]
    for loader in ([resident], mel_only):
        with pytest.raises(ValueError, match="pitch_perturb needs the batch's audio"):
            T_.train_conditioned(Args(), model, step, loader, DEV, 0, pitch_perturb=(-3.0, 3.0))
    for kw in (dict(pitch_perturb=(-13.0, 0.0)), dict(pitch_perturb=(1.0, -1.0)), dict(pitch_perturb=3.0),
               dict(pitch_perturb=(-1.0, 1.0), generator=torch.manual_seed)):
        with pytest.raises(ValueError, match="train_conditioned:"):
            T_.train_conditioned(Args(), model, step, Fixed(), DEV, 0, **kw)
    assert torch.equal(step.opt.flat_param, before)                      # nothing ran


def test_test_conversion_f0_adds_the_psola_row():
    import tests.test_gpu_f0_stats as S                                  # its pair_batch: gliding harmonic tones with a quiet tail
    torch.manual_seed(13)
    model = M.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8).to(DEV).train()
    loader = [S.pair_batch(1, 10240, 11000), S.pair_batch(2, 9000, 8200)]
    stats = np.array([[np.log2(170.0), 0.09], [np.log2(210.0), 0.06]])
    gen = torch.Generator().manual_seed(4)
    angles = [torch.rand(2, (1 + b[0].shape[1] // 256) // 4 * 4, 513, generator=gen).to(DEV) for b in loader]
    plain = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, angles0=angles, f0_stats=stats)
    got = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, angles0=angles, f0_stats=stats, psola_baseline=True)
    assert set(plain) == {"converted", "source", "clips"} and set(got) == set(plain) | {"psola_source"}
    assert str({k: got[k] for k in plain}) == str(plain)                 # the old keys with unchanged values
    row = got["psola_source"]
    assert set(row) == set(plain["source"]) and all(np.isfinite(row[k]) for k in ("f0_rmse_cents", "vuv_error", "f0_corr", "mcd"))
    assert row["stats"] != plain["source"]["stats"]                      # the contour was moved
    same = evaluate.test_conversion_f0(None, model, loader[:1], DEV, 0, iters=2, angles0=angles[:1], psola_baseline=True)      # no statistics: the identity move
    assert abs(same["psola_source"]["f0_rmse_cents"] - same["source"]["f0_rmse_cents"]) < 25.0
