"""GPU tests of the wav -> mel front end (audio.melspectrogram / nsg_audio_melspectrogram, audio.preemphasis) against the
fp64 restatement in tests/helpers/mel_forward64.py, and of its exact properties.  parity unpinned (librosa is absent): what
is pinned is that the kernel computes what the restated formulas say, within a bound derived from the STFT's own.

One figure of the bound differs from how it was first written down: an entry the reference clips to 0 was to compare as
m_gpu <= 1e-5 + delta_b.  1e-5 is the amplitude floor under the logarithm, but the normalised value reaches 0 already at
m = 1e-4 (20 log10 m - 20 + 100 <= 0), so an output of exactly 0 inverts to 1e-4 and no implementation, the fp64 one included,
could meet 1e-5.  The check uses the clip point that the formula has, 1e-4 (mel_forward64.check_amplitude); nothing else is
changed and no entry is left out.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import audio as Au  # noqa: E402
from oracle import audio_oracle as A  # noqa: E402
from tests.helpers import mel_forward64 as H  # noqa: E402

DEV = "cuda:0"


def gpu_mel(y, n_fft=1024, hop=256, n_mels=80, **kw):
    """(n_mels, T) float32 numpy of one clip through the batch form."""
    return Au.melspectrogram(torch.from_numpy(np.ascontiguousarray(y[None])).to(DEV), H.SR, n_fft, hop, n_mels, **kw)[0].cpu().numpy()


@pytest.mark.parametrize("name", ["noise", "harmonic", "sine", "half_zero", "faint"])
def test_matches_the_fp64_restatement(name):
    """Amplitude domain, every entry; output finite and within [0, 1] (the half-zero clip: no log of 0).  On the white noise
    also the normalised domain: every entry is above 5e-4 of the bound's scale (asserted), where the amplitude bound gives
    |d out| <= 0.2 log10(1 + 2e-5 / 5e-4) = 3.4e-3; 3.5e-3 is asserted.  Prints the largest |d out| (recorded in DESIGN.md
    section 5b for the noise and harmonic clips; the same pipeline in fp32 on the CPU, torch.fft.rfft, gives 1.2e-6 and 2.0e-6)."""
    y = H.signals()[name]
    out = gpu_mel(y)
    assert out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
    out_ref, m_ref, delta, _ = H.check_amplitude(out, y, tag=name)
    if name == "noise":
        inside = m_ref >= 5e-4 * (delta / H.REL)
        assert inside.all() and out_ref.min() > 0.0 and out_ref.max() < 1.0, "the cap: every white-noise entry is in the dB-meaningful set"
        d = np.abs(out - out_ref)
        print(f"[noise] normalised domain: max |d out| = {d.max():.3e} over all {d.size} entries (gate 3.5e-3)")
        assert d.max() <= 3.5e-3


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (512, 128), (2048, 512)])
@pytest.mark.parametrize("n_mels", [40, 80])
def test_fft_sizes_mel_counts_and_layouts(n_fft, hop, n_mels):
    rs = np.random.RandomState(n_fft + n_mels)
    y = np.stack([H.rescale(rs.randn(hop * 19)) for _ in range(2)])
    yd = torch.from_numpy(y).to(DEV)
    a = Au.melspectrogram(yd, H.SR, n_fft, hop, n_mels)
    b = Au.melspectrogram(yd, H.SR, n_fft, hop, n_mels, layout="frame_major")
    assert tuple(a.shape) == (2, n_mels, 20) and tuple(b.shape) == (2, 20, n_mels)
    assert torch.equal(a, b.transpose(1, 2)), "the two layouts are transposes of each other bit for bit"
    for i in range(2):
        H.check_amplitude(a[i].cpu().numpy(), y[i], n_fft, hop, n_mels, tag=f"{n_fft}/{hop}/{n_mels}/{i}")


def test_ragged_batch_is_each_clip_alone_bit_for_bit():
    hop = 256
    lens = [256 * 63, 256 * 63 + 1, 256 * 63 + 255, 256 * 40, 600]
    L = max(lens)
    rs = np.random.RandomState(4)
    batch = np.zeros((len(lens), L), dtype=np.float32)
    for i, n in enumerate(lens):
        batch[i, :n] = H.rescale(rs.randn(n))
    T = 1 + L // hop
    for layout in ("mel_major", "frame_major"):
        got = Au.melspectrogram(torch.from_numpy(batch).to(DEV), lengths=torch.tensor(lens), layout=layout).cpu().numpy()
        if layout == "frame_major":
            got = got.transpose(0, 2, 1)
        assert got.shape == (len(lens), 80, T)
        for i, (n, Tb) in enumerate(zip(lens, (64, 64, 64, 41, 3))):
            assert Tb == 1 + n // hop
            alone = gpu_mel(batch[i, :n].copy(), layout="mel_major")
            assert alone.shape == (80, Tb)
            assert np.array_equal(got[i, :, :Tb], alone), (layout, i)
            assert (got[i, :, Tb:] == 0).all(), (layout, i)
            H.check_amplitude(alone, batch[i, :n], tag=f"ragged {n}")
    # lengths as a list / numpy / GPU tensor are the same call; lengths=None is every clip at L
    full = Au.melspectrogram(torch.from_numpy(batch).to(DEV))
    same = Au.melspectrogram(torch.from_numpy(batch).to(DEV), lengths=np.full(len(lens), L))
    assert torch.equal(full, same)


def test_numpy_form_zero_clip_and_range():
    y = H.signals()["harmonic"]
    m = Au.melspectrogram(y, 22050, 1024, 256, 80)                                    # the reference's call
    assert isinstance(m, np.ndarray) and m.dtype == np.float32 and m.shape == (80, 64)
    assert np.array_equal(m, gpu_mel(y))
    assert np.array_equal(Au.melspectrogram(y.astype(np.float64), layout="frame_major"), m.T)
    z = Au.melspectrogram(torch.zeros(2, 256 * 10, device=DEV))
    assert tuple(z.shape) == (2, 80, 11) and (z == 0).all(), "floor -> -100 dB - 20 -> clipped to exactly 0"


def test_preemphasis_and_its_inverse():
    rs = np.random.RandomState(6)
    x = rs.randn(3, 7000).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    p = Au.preemphasis(xd)
    want = x.astype(np.float64).copy()
    want[:, 1:] -= 0.97 * x[:, :-1].astype(np.float64)
    np.testing.assert_allclose(p.cpu().numpy(), want, rtol=0, atol=4e-7 * np.abs(x).max())     # two fp32 roundings of values <= 2 max|x|
    back = Au.inv_preemphasis(p).cpu().numpy()
    np.testing.assert_allclose(back, x, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("name", ["noise", "harmonic"])
def test_round_trip_through_the_export(name):
    """melspectrogram(inv_mel_spectrogram(melspectrogram(y))) against melspectrogram(y), mean absolute difference in
    normalised units: a sanity bound (the export raises magnitudes to the power 1.5 and Griffin-Lim is lossy).  The value it is
    held to is recomputed here from the fp64 restatements alone, with the same initial phases; the GPU path must land within
    25 % of it either way.  (fp64, white noise: 0.0428.)"""
    y = H.signals(256 * 23)[name]
    u = np.random.RandomState(11).rand(513, 24)
    m0 = H.forward64(y)[0]
    m1 = H.forward64(A.inv_mel_spectrogram(m0, H.SR, 1024, 256, 80, angles0=u))[0]
    d_ref = float(np.abs(m1 - m0).mean())
    g0 = Au.melspectrogram(y)
    w = Au.inv_mel_spectrogram(g0, H.SR, 1024, 256, 80, angles0=np.ascontiguousarray(u.T[None], dtype=np.float32))
    assert w.shape == (256 * 23,) and np.isfinite(w).all()
    g1 = Au.melspectrogram(w)
    d_gpu = float(np.abs(g1 - g0).mean())
    print(f"[{name}] round trip mean |d mel|: fp64 restatement {d_ref:.4f}, GPU {d_gpu:.4f}")
    assert abs(d_gpu - d_ref) <= 0.25 * d_ref
