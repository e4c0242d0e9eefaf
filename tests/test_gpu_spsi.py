"""GPU tests of the single-pass spectrogram inversion phases (csrc/audio.hip: spsi_frames_kernel, spsi_walk_kernel; include/nsg.h:
nsg_audio_spsi_phases) and of their wiring through audio.py and evaluate.py.

The reference is the numpy fp64 restatement tests/helpers/spsi_ref.py.  Every operation of the definition is a correctly rounded
IEEE operation or an exact product by a power of two, so the expectation is bit-for-bit equality of the angles, every element,
every shape and pattern.  A second run of the kernels is the reference only where determinism is the property.  The convergence
relations of the last test are confirmed in fp64 by tests/test_spsi_host.py for the same signal and seed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio as Au, evaluate, models, ops  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import spsi_ref as R  # noqa: E402
from tests.helpers.guarded_ws import GuardedWorkspace  # noqa: E402

DEV = "cuda:0"
TS, BS = (1, 2, 3, 33), (1, 3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.view(torch.int32)


def circular(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.minimum(d, 1.0 - d)


# ----------------------------------------------------------------------------------------------------------------------
# against the restatement, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", R.NFFTS)
@pytest.mark.parametrize("hop_of", ["n_fft", "n_fft/4", "32"])
def test_the_angles_are_the_restatements_bit_for_bit(n_fft, hop_of):
    """Every pattern of spsi_ref.patterns at T in {1, 2, 3, 33} and B in {1, 3}: equal bits, every element; the batch of one is clip
    0 of the batch of three; two launches agree."""
    hop = {"n_fft": n_fft, "n_fft/4": n_fft // 4, "32": 32}[hop_of]
    F = n_fft // 2 + 1
    bad = []
    for T in TS:
        pats = R.patterns(n_fft, T, max(BS))
        assert len(pats) == 11
        for name, S in pats.items():
            assert S.shape == (3, T, F) and S.dtype == np.float32 and np.isfinite(S).all()
            want = R.spsi_batch(S, n_fft, hop)
            assert want.min() >= 0.0 and want.max() < 1.0
            for B in BS:
                Sd = dev(S[:B])
                got = Au.spsi_phases(Sd, n_fft, hop)
                assert got.dtype == torch.float32 and tuple(got.shape) == (B, T, F) and got.device == Sd.device
                assert torch.equal(bits(got), bits(Au.spsi_phases(Sd, n_fft, hop))), (name, T, B)          # two runs
                g = got.cpu().numpy()
                ne = g.view(np.int32) != want[:B].view(np.int32)
                if ne.any():
                    dist = float(circular(g, want[:B]).max())
                    print(f"[{n_fft}/{hop} T={T} B={B} {name}] {int(ne.sum())} of {ne.size} elements differ, circular distance {dist:.3e} turns, "
                          f"first at {tuple(int(i) for i in np.argwhere(ne)[0])}")
                    bad.append((name, T, B, int(ne.sum()), dist))
    assert not bad, bad


def test_each_clip_of_a_batch_is_what_it_is_alone():
    n_fft, hop, T = 1024, 256, 33
    pats = R.patterns(n_fft, T, 3)
    S = np.concatenate([pats["random"], pats["alternating"], pats["moving_peak"], pats["denormal_and_huge"]])
    got = Au.spsi_phases(dev(S), n_fft, hop)
    for b in range(len(S)):
        assert torch.equal(bits(got[b:b + 1]), bits(Au.spsi_phases(dev(S[b:b + 1]), n_fft, hop))), b


def test_a_long_clip_keeps_its_phase():
    """900 frames, the export's length: the fp64 turns, reduced every frame, are the restatement's bits to the end."""
    n_fft, hop, T = 1024, 256, 900
    S = np.abs(R.stft(R.harmonic_signal(n_fft, hop, T, 29), n_fft, hop)).astype(np.float32).T[None]
    got = Au.spsi_phases(dev(S), n_fft, hop).cpu().numpy()
    assert np.array_equal(got.view(np.int32), R.spsi_batch(S, n_fft, hop).view(np.int32))


# ----------------------------------------------------------------------------------------------------------------------
# the workspace
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,T,B", [(512, 128, 1, 1), (1024, 256, 3, 3), (2048, 32, 33, 2)])
def test_spsi_on_an_exact_size_poisoned_workspace(monkeypatch, n_fft, hop, T, B):
    """Exactly nsg_audio_griffin_lim_workspace_bytes bytes between guards, filled with 0x00 and with 0xFF (an owner of 65535 if it were
    read unwritten), and the angles exactly their size between guards of their own; one byte fewer is refused."""
    F = n_fft // 2 + 1
    S = dev(R.patterns(n_fft, T, 3)["random"][:B])
    want = Au.spsi_phases(S, n_fft, hop)
    need = _lib.query("nsg_audio_griffin_lim_workspace_bytes", B, T, n_fft)
    for fill in (0x00, 0xFF):
        ws, out = GuardedWorkspace(fill), GuardedWorkspace(0xFF)
        monkeypatch.setattr(ops, "WS", ws)
        angles = out.get(B * T * F * 4, torch.device(DEV)).view(torch.float32).view(B, T, F)
        buf, nb = ops._ws(S.device, "nsg_audio_griffin_lim_workspace_bytes", B, T, n_fft)
        _lib.call("nsg_audio_spsi_phases", _p(S), _p(angles), B, T, n_fft, hop, _p(buf), nb, _stream())
        ws.verify()
        out.verify()
        assert ws.sizes == [need] and nb == need
        assert torch.equal(bits(angles), bits(want)), fill
        with pytest.raises(_lib.NsgError, match="nsg_audio_spsi_phases: workspace too small"):
            _lib.call("nsg_audio_spsi_phases", _p(S), _p(angles), B, T, n_fft, hop, _p(buf), need - 1, _stream())
        assert torch.equal(bits(angles), bits(want))


# ----------------------------------------------------------------------------------------------------------------------
# wiring
# ----------------------------------------------------------------------------------------------------------------------
def test_inv_mel_spectrogram_with_init_spsi_is_its_pieces():
    rs = np.random.RandomState(5)
    mel = dev(rs.rand(2, 80, 12).astype(np.float32))
    S = Au.mel_to_linear(mel)
    for k, momentum in ((0, 0.0), (3, 0.0), (3, 0.99)):
        got = Au.inv_mel_spectrogram(mel, iters=k, init="spsi", momentum=momentum)
        want = Au.inv_preemphasis(Au.griffin_lim(S, 1024, 256, k, angles0=Au.spsi_phases(S, 1024, 256), momentum=momentum))
        assert torch.equal(bits(got), bits(want)), (k, momentum)
    one = Au.inv_mel_spectrogram(mel[0].cpu().numpy(), iters=3, init="spsi")
    assert np.array_equal(one, Au.inv_mel_spectrogram(mel, iters=3, init="spsi")[0].cpu().numpy())
    # the default is the path there was
    a0 = dev(rs.rand(2, 12, 513).astype(np.float32))
    plain = Au.inv_mel_spectrogram(mel, iters=3, angles0=a0)
    assert torch.equal(bits(Au.inv_mel_spectrogram(mel, iters=3, angles0=a0, init="random")), bits(plain))
    assert torch.equal(bits(plain), bits(Au.inv_preemphasis(Au.griffin_lim(S, 1024, 256, 3, a0))))
    assert not torch.equal(plain, Au.inv_mel_spectrogram(mel, iters=3, init="spsi"))


def test_test_conversion_f0_passes_init_through(capsys):
    from tests.test_gpu_f0_stats import HOP, pair_batch
    torch.manual_seed(13)
    model = models.VQVAE(1, 16, 32, n_speakers=2).to(DEV).eval()
    loader = [pair_batch(1, 10240, 11000)]
    got = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, init="spsi")
    assert "init spsi" in capsys.readouterr().out
    ws, ls, _, _, g = loader[0]
    mel_s = Au.melspectrogram(ws.to(DEV), lengths=ls)
    Tc = mel_s.shape[2] // 4 * 4
    _, conv = evaluate.convert_voice(model, mel_s[:, :, :Tc].contiguous(), g)
    S = Au.mel_to_linear(conv.squeeze(1).contiguous())
    y = Au.griffin_lim(S, 1024, HOP, 2, Au.spsi_phases(S, 1024, HOP))
    assert got["converted"]["spectral_convergence"] == pytest.approx(float(Au.spectral_convergence(y, S, 1024, HOP).mean()), rel=1e-12)
    a0 = torch.rand(2, Tc, 513, generator=torch.Generator().manual_seed(4)).to(DEV)
    plain = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, angles0=a0)
    assert "init random" in capsys.readouterr().out
    assert str(plain) == str(evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=2, angles0=a0, init="random"))


# ----------------------------------------------------------------------------------------------------------------------
# the point of the feature
# ----------------------------------------------------------------------------------------------------------------------
def test_spsi_phases_start_griffin_lim_closer_than_random_ones():
    """The harmonic signal of tests/test_spsi_host.py (fp64 there: 0.092 against 0.638 at 0 iterations, 0.064 against 0.289 at 4), on
    the kernels: relations only."""
    S64, u64 = R.trial_case(**R.POINT)
    n, h = R.POINT["n_fft"], R.POINT["hop"]
    S, u = dev(S64.T.astype(np.float32)[None]), dev(u64.T.astype(np.float32)[None])
    a = Au.spsi_phases(S, n, h)
    sc = {(name, k): float(Au.spectral_convergence(Au.griffin_lim(S, n, h, k, a0), S, n, h)) for name, a0 in (("random", u), ("spsi", a)) for k in (0, 4)}
    print("  ".join(f"{name} x {k}: {v:.4f}" for (name, k), v in sc.items()))
    assert sc["spsi", 0] < sc["random", 0] and sc["spsi", 4] < sc["random", 4]
    assert sc["spsi", 0] < 0.5 * sc["random", 0]
