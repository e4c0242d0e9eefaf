"""The layers above nsg_dtw: nsg_mel_cepstra against its fp32 restatement bit for bit, audio.mel_cepstral_distortion against
exact cases and an independent fp64 computation, evaluate.convert_voice against the model's own encode / decode, and
evaluate.test_conversion against per-clip values.  Guarded buffers as in test_gpu_dtw.py."""
import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, evaluate, models, ops
from tests.helpers import dtw_ref as R

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)
DEV = torch.device("cuda:0")
GUARD = 67


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def guarded_mel(host, frames=None):
    """host (B, n_mels, T) as a view into a NaN-filled buffer; with frames, NaN at and past each clip's count."""
    host = host.copy()
    if frames is not None:
        for b, f in enumerate(frames):
            host[b, :, f:] = np.nan
    buf = torch.full((host.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + host.size].view(*host.shape)
    view.copy_(torch.from_numpy(host))
    return view


@pytest.mark.parametrize("with_frames", [False, True])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 333])
@pytest.mark.parametrize("n_mels,K", [(80, 13), (13, 12), (80, 64), (128, 1)])
def test_mel_cepstra_matches_the_restatement(n_mels, K, T, with_frames):
    B = 3
    rs = np.random.RandomState(n_mels + K + T)
    host = rs.random_sample((B, n_mels, T)).astype(np.float32)
    host[:, ::5, ::3] *= -1                                               # signs: nothing in the definition needs mels >= 0
    table = audio.cepstra_table(n_mels, K) if K < n_mels else rs.standard_normal((K, n_mels)).astype(np.float32)
    frames = [T, 0, max(0, T - 2)] if with_frames else None
    mel = guarded_mel(host, frames)
    obuf = torch.full((B * T * K + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    out = obuf[GUARD:GUARD + B * T * K].view(B, T, K)
    got = ops.mel_cepstra(mel, torch.from_numpy(table).to(DEV), frames, out=out)
    assert got is out
    whole = obuf.cpu().numpy()
    assert np.isnan(whole[:GUARD]).all() and np.isnan(whole[GUARD + out.numel():]).all(), "a store outside c"
    c = whole[GUARD:GUARD + out.numel()].reshape(B, T, K)
    for b in range(B):
        f = frames[b] if with_frames else T
        want = R.cepstra32(host[b], table, f)
        assert np.array_equal(bits(c[b]), bits(want)), (b, int((bits(c[b]) != bits(want)).sum()))
        assert (bits(c[b, f:]) == 0).all()                               # the padding is +0.0 by bit pattern
    if with_frames:                                                       # the same counts as an int32 tensor on the device
        again = ops.mel_cepstra(mel, torch.from_numpy(table).to(DEV), torch.tensor(frames, dtype=torch.int32, device=DEV))
        assert np.array_equal(bits(again.cpu().numpy()), bits(c))


def test_audio_mel_cepstra_shapes_and_table():
    rs = np.random.RandomState(5)
    host = rs.random_sample((2, 80, 70)).astype(np.float32)
    mel = torch.from_numpy(host).to(DEV)
    c3, c4 = audio.mel_cepstra(mel), audio.mel_cepstra(mel.unsqueeze(1), frames=[70, 33])
    assert tuple(c3.shape) == (2, 70, 13) and torch.equal(c3[0], c4[0]) and torch.equal(c3[1, :33], c4[1, :33]) and not c4[1, 33:].any()
    assert np.array_equal(bits(c3[1].cpu().numpy()), bits(R.cepstra32(host[1], audio.cepstra_table(80, 13))))
    shifted = audio.mel_cepstra(mel + 0.25)                               # a level change moves c0 only, which is left out
    assert (shifted - c3).abs().max() < 1e-4 * c3.abs().max()
    with pytest.raises(ValueError, match="n_ceps"):
        audio.mel_cepstra(mel, n_ceps=80)
    with pytest.raises(ValueError, match="expected a mel tensor"):
        audio.mel_cepstra(mel[0])
    with pytest.raises(_lib.NsgError, match=r"frames: every length must be in \[0, 70\]"):
        audio.mel_cepstra(mel, frames=[70, 71])


def test_mcd_of_a_mel_against_itself_and_a_stretched_copy():
    rs = np.random.RandomState(6)
    T = 90
    host = rs.random_sample((2, 80, T)).astype(np.float32)
    frames = [T, 57]
    mel = guarded_mel(host, frames)
    mcd, steps = audio.mel_cepstral_distortion(mel, mel, frames, frames)
    assert mcd.dtype == torch.float32 and steps.dtype == torch.int32
    assert (bits(mcd.cpu().numpy()) == 0).all() and steps.tolist() == frames
    # every second frame repeated: the warp absorbs it exactly
    idx = np.repeat(np.arange(T), np.where(np.arange(T) % 2 == 1, 2, 1))
    longer = [int((idx < f).sum()) for f in frames]
    stretched = guarded_mel(host[:, :, idx], longer)
    for x, y, fx, fy in ((mel, stretched, frames, longer), (stretched, mel, longer, frames)):
        mcd, steps = audio.mel_cepstral_distortion(x, y, fx, fy)
        assert (bits(mcd.cpu().numpy()) == 0).all() and steps.tolist() == longer
    with pytest.raises(_lib.NsgError, match=r"frames_a: every length must be in \[1, 90\]"):
        audio.mel_cepstral_distortion(mel, mel, [0, 5], frames)


@pytest.mark.parametrize("la,lb", [(65, 64), (129, 200), (37, 150)])
def test_mcd_against_fp64(la, lb):
    """Bound, relative: (n_mels + la + lb + 64) * 2^-23.  A cepstral coefficient is an fp32 chain of n_mels products and sums: its
    error is at most about n_mels * 2^-24 of sum_j |mel_j table_kj|, and the coefficients' errors carry into a frame distance
    (a difference of such vectors, whose own K-term chain and correctly rounded root add a few ulp) at no more than that
    magnitude relative to the distances these inputs have, which are of the size of the coefficients themselves.  The cost along
    a path sums at most la + lb - 1 distances with one rounding each, (la + lb) * 2^-24 relative, and the minimum over paths is
    1-Lipschitz in a uniform per-path perturbation (as for the fp32 restatement, tests/test_dtw_host.py).  The quotient by steps
    and the product with the constant are two more roundings.  Together about (n_mels + la + lb + a few) * 2^-24; the bound
    leaves a factor of two and 64 ulp.  The fp64 side takes the kernel's own steps: the figure is cost / steps and a different
    but equally cheap path may be longer."""
    n_mels, K = 80, 13
    rs = np.random.RandomState(la + lb)
    ha, hb = rs.random_sample((1, n_mels, la + 4)).astype(np.float32), rs.random_sample((1, n_mels, lb + 1)).astype(np.float32)
    mcd, steps = audio.mel_cepstral_distortion(guarded_mel(ha, [la]), guarded_mel(hb, [lb]), [la], [lb], n_ceps=K)
    t64 = R.dct_table64(n_mels, K)
    c64, _, _ = R.dtw64(R.cepstra64(ha[0, :, :la], t64), R.cepstra64(hb[0, :, :lb], t64))
    want = (10.0 * np.sqrt(2.0) / np.log(10.0)) * c64 / int(steps[0])
    rel = abs(float(mcd[0]) - want) / want
    print(f"mcd {float(mcd[0]):.6f} dB, fp64 {want:.6f} dB, relative error {rel:.3e}, bound {(n_mels + la + lb + 64) * 2.0 ** -23:.3e}")
    assert max(la, lb) <= int(steps[0]) <= la + lb - 1
    assert rel <= (n_mels + la + lb + 64) * 2.0 ** -23


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return models.VQVAE(1, 16, 32, n_speakers=3).to(DEV).train()


def test_convert_voice(model):
    mel = torch.rand(2, 1, 80, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    g = torch.tensor([2, 0], dtype=torch.int64)
    for training in (True, False):
        model.train(training)
        codes, out = evaluate.convert_voice(model, mel, g)
        assert model.training is training
        assert tuple(codes.shape) == (2, 20, 16) and codes.dtype == torch.int64 and tuple(out.shape) == (2, 1, 80, 64)
        model.eval()
        with torch.no_grad():
            want_codes = model.encode(mel)
            want = model.decode(want_codes, g.to(DEV))
        assert torch.equal(codes, want_codes) and torch.equal(out, want)
    model.train()
    _, other = evaluate.convert_voice(model, mel.squeeze(1), torch.tensor([1, 0], dtype=torch.int64, device=DEV))
    assert not torch.equal(other[0], out[0])                              # another target speaker, another mel
    with pytest.raises(ValueError, match="g_target"):
        evaluate.convert_voice(model, mel, torch.tensor([0, 3]))
    assert model.training


def test_test_conversion_is_the_clip_weighted_mean(model, capsys):
    rs = np.random.RandomState(8)

    def batch(B, Ts, Tt, seed):
        g = torch.Generator().manual_seed(seed)
        fs = rs.randint(Ts // 2, Ts + 1, B)
        ft = rs.randint(Tt // 2, Tt + 1, B)
        fs[0], ft[0] = Ts, Tt
        return (torch.rand(B, 80, Ts, generator=g), torch.from_numpy(fs), torch.rand(B, 80, Tt, generator=g), torch.from_numpy(ft),
                torch.from_numpy(rs.randint(0, 3, B).astype(np.int64)))

    loader = [batch(3, 70, 81, 1), batch(2, 48, 40, 2)]                   # 70 frames: the converted mel has 68
    model.train()
    got_c, got_s = evaluate.test_conversion(None, model, loader, DEV, 0)
    assert model.training and "Conversion test set" in capsys.readouterr().out
    conv, src = [], []
    for c_src, fs, c_tgt, ft, g in loader:
        Ts = c_src.shape[2] // 4 * 4
        _, out = evaluate.convert_voice(model, c_src[:, :, :Ts].contiguous().to(DEV), g)
        assert out.shape[3] == Ts
        conv += audio.mel_cepstral_distortion(out, c_tgt.to(DEV), np.minimum(fs.numpy(), Ts) // 4 * 4, ft)[0].double().tolist()
        src += audio.mel_cepstral_distortion(c_src.to(DEV), c_tgt.to(DEV), fs, ft)[0].double().tolist()
    assert len(conv) == 5 and min(conv) > 0 and min(src) > 0
    assert abs(got_c - np.mean(conv)) <= 1e-12 * np.mean(conv) and abs(got_s - np.mean(src)) <= 1e-12 * np.mean(src)
    assert abs(got_c - (np.mean(conv[:3]) + np.mean(conv[3:])) / 2) > 1e-6 * got_c       # not the mean of the batch means
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.test_conversion(None, model, [], DEV, 0)
