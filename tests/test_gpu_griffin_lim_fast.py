"""GPU tests of fast Griffin-Lim and the spectral-convergence figure (csrc/audio.hip: stft_kernel's momentum outputs, the
convergence_* kernels; include/nsg.h: nsg_audio_griffin_lim_fast, nsg_audio_spectral_convergence) and of their wiring through
audio.py and evaluate.py.

Every comparison is against the fp64 restatement tests/helpers/griffin_lim_fast_ref.py (built on oracle/audio_oracle.py's stft /
istft) or an exact identity; a second run of the code under test is the reference only where bit-equality is the property.  The
bounds are audio_envelope's yardstick (512 x the restatement's own response to a 2^-24 perturbation of S, at the same momentum)
and griffin_lim_fast_ref.sc_eps, both checked reachable on the CPU by tests/test_griffin_lim_fast_host.py.  Each test prints its
figures before it asserts; the kernels' measured shares of each bound are recorded in DESIGN.md section 5j."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, audio as Au, evaluate, models, ops  # noqa: E402
from neural_sound_generation_amd.ops import _p, _stream  # noqa: E402
from tests.helpers import audio_envelope as E, griffin_lim_fast_ref as R  # noqa: E402
from tests.helpers.guarded_ws import GuardedWorkspace  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def state_like(S, fill):
    return torch.full(tuple(S.shape), complex(fill, fill), dtype=torch.complex64, device=S.device)


def raw_fast(S, u, n_fft, hop, iters, momentum, c, y=None):
    """nsg_audio_griffin_lim_fast through the binding, with the caller's c (a float32 (B, T, F, 2) tensor or None = NULL) and y."""
    B, T, F = S.shape
    y = torch.empty(B, hop * (T - 1), dtype=torch.float32, device=S.device) if y is None else y
    ws, nb = ops._ws(S.device, "nsg_audio_griffin_lim_workspace_bytes", B, T, n_fft)
    _lib.call("nsg_audio_griffin_lim_fast", _p(S), _p(u), _p(y), _p(c), B, T, n_fft, hop, iters, float(momentum), _p(ws), nb, _stream())
    return y


def bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# against the fp64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def check_fast(S, u, n_fft, hop, tag, zero_clips=()):
    """S, u (B, T, F) float32.  For iterations {1, 3} x momentum {0.5, 0.99} and every clip: max|y - y64| <= 512 x (the restatement's
    largest response to S (1 + 2^-24 r)) x max|y64|.  The state c is held to X_iters the same way, relative to max|X_iters|, on the
    grid nsg_audio_stft does not take (hop (T - 1) <= n_fft / 2); on every other grid it is held bit for bit to the device's own
    stft of y_{iters-1} (state_is_the_stft) and the fp64 comparison is printed only: with hop == n_fft the frames do not overlap,
    a perturbation of S moves t = X + momentum (X - X_prev) almost radially, and the response of X to S says little about a
    rounding that turns a nearly cancelled t (507 x at 1024/1024, |t| = 1e-4 |X| in one bin)."""
    B, T, F = S.shape
    hold_state = hop * (T - 1) <= n_fft // 2
    Sd, ud = dev(S), dev(u)
    rows = []
    for momentum in R.GL_FAST_MOMENTA:
        for iters in R.GL_FAST_ITERS:
            c = state_like(Sd, NAN)
            y = Au.griffin_lim(Sd, n_fft, hop, iters, ud, momentum=momentum, state=c).cpu().numpy()
            c = c.cpu().numpy()
            assert y.shape == (B, hop * (T - 1)) and np.isfinite(y).all() and np.isfinite(c.view(np.float32)).all(), (tag, iters, momentum)
            for b in range(B):
                want, X, resp, resp_x = R.gl_fast_response(S[b].T.astype(np.float64), n_fft, hop, iters, u[b].T.astype(np.float64), momentum)
                peak, peak_x = float(np.abs(want).max()), float(np.abs(X).max())
                err, err_x = float(np.abs(y[b] - want).max()), float(np.abs(c[b].T - X).max())
                rows.append((momentum, iters, b, err, peak, resp, err_x, peak_x, resp_x))
                if b in zero_clips:
                    assert peak == 0.0 and peak_x == 0.0
                    continue
                print(f"[{tag}] momentum={momentum} iters={iters} clip={b}: y err/max={err / peak:.3e} response={resp:.3e} ratio={err / peak / resp:.1f}; "
                      f"c err/max={err_x / peak_x:.3e} response={resp_x:.3e} ratio={err_x / peak_x / resp_x:.1f} (allowed {E.GL_MULTIPLE:.0f})")
    for momentum, iters, b, err, peak, resp, err_x, peak_x, resp_x in rows:
        assert err <= E.GL_MULTIPLE * resp * peak, (tag, momentum, iters, b, err / max(peak, 1e-300), resp)
        if hold_state or peak_x == 0.0:
            assert err_x <= E.GL_MULTIPLE * resp_x * peak_x, (tag, momentum, iters, b, err_x / max(peak_x, 1e-300), resp_x)
    if not hold_state:
        state_is_the_stft(Sd, ud, n_fft, hop, (1, 3))
    return rows


def state_is_the_stft(S, u, n_fft, hop, iters_list):
    """c = X_iters = stft(y_{iters-1}), bit for bit: nsg_audio_stft runs the same load and FFT code (hop (T - 1) > n_fft / 2)."""
    for momentum in R.GL_FAST_MOMENTA:
        for iters in iters_list:
            c = state_like(S, NAN)
            Au.griffin_lim(S, n_fft, hop, iters, u, momentum=momentum, state=c)
            X = Au.stft(Au.griffin_lim(S, n_fft, hop, iters - 1, u, momentum=momentum), n_fft, hop)
            assert X.shape == c.shape and torch.equal(bits(X), bits(c)), (n_fft, hop, momentum, iters)


@pytest.mark.parametrize("n_fft,hop,T", R.GL_FAST_CASES)
def test_fast_griffin_lim_matches_the_restatement(n_fft, hop, T):
    S, u = E.gl_case(n_fft, hop, T)
    check_fast(S, u, n_fft, hop, f"glf {n_fft}/{hop} T={T}")


@pytest.mark.parametrize("n_fft,T", [(512, 5), (2048, 6)])
def test_fast_griffin_lim_degenerate_magnitudes(n_fft, T):
    """All-zero frames, all-zero bins and an all-zero clip: within the same bound, and the zero clip exactly zero with a zero state
    (X = prev = 0 gives t = 0: the np.angle(0) = 0 branch, times S = 0)."""
    S, u = E.degenerate_case(n_fft, T)
    check_fast(S, u, n_fft, n_fft // 4, f"glf degenerate {n_fft} T={T}", zero_clips=(2,))
    for iters in (1, 3):
        c = state_like(dev(S), NAN)
        y = Au.griffin_lim(dev(S), n_fft, n_fft // 4, iters, dev(u), momentum=0.99, state=c)
        assert (y[2] == 0).all() and (torch.view_as_real(c[2]) == 0).all(), iters
        alone = Au.griffin_lim(dev(S[2:]), n_fft, n_fft // 4, iters, dev(u[2:]), momentum=0.99)
        assert (alone == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# exact statements
# ----------------------------------------------------------------------------------------------------------------------
EXACT = [(512, 128, 2), (1024, 256, 24), (2048, 512, 9)]


@pytest.mark.parametrize("n_fft,hop,T", EXACT)
def test_momentum_zero_is_griffin_lim_bit_for_bit_without_a_state_buffer(n_fft, hop, T):
    S, u = (dev(a) for a in E.gl_case(n_fft, hop, T))
    for iters in (0, 1, 3):
        want = Au.griffin_lim(S, n_fft, hop, iters, u)
        assert torch.equal(raw_fast(S, u, n_fft, hop, iters, 0.0, None), want)
        c = torch.full((*S.shape, 2), NAN, device=DEV)
        assert torch.equal(raw_fast(S, u, n_fft, hop, iters, 0.0, c), want) and bool(torch.isnan(c).all())      # given, c is not touched
        assert torch.equal(Au.griffin_lim(S, n_fft, hop, iters, u, momentum=0.0), want)
        assert torch.equal(Au.griffin_lim(S, n_fft, hop, iters, u, momentum=1e-50), want)                         # 0.f to the kernel: the plain path
    with pytest.raises(ValueError, match="state goes with momentum > 0"):
        Au.griffin_lim(S, n_fft, hop, 1, u, momentum=1e-50, state=state_like(S, NAN))


@pytest.mark.parametrize("n_fft,hop,T", EXACT)
def test_zero_iterations_leave_the_state_untouched(n_fft, hop, T):
    S, u = (dev(a) for a in E.gl_case(n_fft, hop, T))
    c = torch.full((*S.shape, 2), NAN, device=DEV)
    y = raw_fast(S, u, n_fft, hop, 0, 0.99, c)
    assert bool(torch.isnan(c).all()) and torch.equal(y, Au.griffin_lim(S, n_fft, hop, 0, u))


@pytest.mark.parametrize("n_fft,hop,T", [(512, 128, 5), (512, 64, 9), (1024, 256, 24), (2048, 512, 9), (1024, 1024, 4)])
def test_the_state_is_the_stft_of_the_last_but_one_waveform(n_fft, hop, T):
    """Iterations 1, 2 and 4 at both momenta, on every grid of the list that nsg_audio_stft takes (on the short grid 512/128 T=2 the
    state is held to the restatement by check_fast)."""
    S, u = (dev(a) for a in E.gl_case(n_fft, hop, T))
    state_is_the_stft(S, u, n_fft, hop, (1, 2, 4))


@pytest.mark.parametrize("n_fft,hop,T", EXACT)
def test_the_state_on_entry_is_never_read_and_launches_repeat(n_fft, hop, T):
    S, u = (dev(a) for a in E.gl_case(n_fft, hop, T))
    for iters in (1, 3):
        runs = []
        for fill in (NAN, 0.0, NAN):
            c = state_like(S, fill)
            runs.append((Au.griffin_lim(S, n_fft, hop, iters, u, momentum=0.99, state=c), c))
        for y, c in runs[1:]:
            assert torch.equal(bits(y), bits(runs[0][0])) and torch.equal(bits(c), bits(runs[0][1])), iters
        for b in range(S.shape[0]):                                           # a clip alone is the clip in the batch
            c1 = state_like(S[b:b + 1], NAN)
            y1 = Au.griffin_lim(S[b:b + 1].contiguous(), n_fft, hop, iters, u[b:b + 1].contiguous(), momentum=0.99, state=c1)
            assert torch.equal(bits(y1[0]), bits(runs[0][0][b])) and torch.equal(bits(c1[0]), bits(runs[0][1][b])), (iters, b)


# ----------------------------------------------------------------------------------------------------------------------
# the workspace contract
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,T", [(512, 128, 2), (512, 128, 5), (1024, 256, 24)])
def test_fast_griffin_lim_on_an_exact_size_poisoned_workspace(monkeypatch, n_fft, hop, T):
    """Exactly nsg_audio_griffin_lim_workspace_bytes bytes between guards, filled with 0x00 and with 0xFF (NaN), and y and c exactly
    their sizes between guards of their own: no guard byte changes and the result does not depend on the fill."""
    S, u = (dev(a) for a in E.gl_case(n_fft, hop, T))
    B, _, F = S.shape
    want_c = state_like(S, NAN)
    want_y = Au.griffin_lim(S, n_fft, hop, 3, u, momentum=0.99, state=want_c)
    need = _lib.query("nsg_audio_griffin_lim_workspace_bytes", B, T, n_fft)
    for fill in (0x00, 0xFF):
        ws, out = GuardedWorkspace(fill), GuardedWorkspace(0xFF)
        monkeypatch.setattr(ops, "WS", ws)
        y = out.get(B * hop * (T - 1) * 4, torch.device(DEV)).view(torch.float32).view(B, hop * (T - 1))
        c = out.get(B * T * F * 8, torch.device(DEV)).view(torch.float32).view(B, T, F, 2)
        raw_fast(S, u, n_fft, hop, 3, 0.99, c, y)
        ws.verify()
        out.verify()
        assert ws.sizes == [need], (ws.sizes, need)
        assert torch.equal(bits(y), bits(want_y)) and torch.equal(bits(c), bits(torch.view_as_real(want_c))), fill


# ----------------------------------------------------------------------------------------------------------------------
# the point of the feature
# ----------------------------------------------------------------------------------------------------------------------
def test_sixteen_fast_iterations_beat_sixty_plain_ones():
    """The host test's harmonic signal (fp64 there: 0.164 plain x 60, 0.141 at 0.99 x 16, 0.079 at 0.99 x 60), measured by
    audio.spectral_convergence on the kernels' own waveforms."""
    _, S64, u64 = R.harmonic_case()
    S, u = dev(S64.T.astype(np.float32)[None]), dev(u64.T.astype(np.float32)[None])
    n, h = R.HARM_NFFT, R.HARM_HOP
    sc = {(m, k): float(Au.spectral_convergence(Au.griffin_lim(S, n, h, k, u, momentum=m), S, n, h)) for m, k in ((0.0, 60), (0.99, 16), (0.99, 60))}
    print(f"plain x 60: {sc[0.0, 60]:.4f}   0.99 x 16: {sc[0.99, 16]:.4f}   0.99 x 60: {sc[0.99, 60]:.4f}")
    assert sc[0.99, 16] < sc[0.0, 60] and sc[0.99, 60] < sc[0.0, 60]


# ----------------------------------------------------------------------------------------------------------------------
# audio.spectral_convergence
# ----------------------------------------------------------------------------------------------------------------------
def check_convergence(y, S, n_fft, hop, tag):
    """y (B, L), S (B, T, F) float32 on the host: the device's figure against fp64 within sc_eps (1 + sc_64); the frames' sums add up
    to the clips'; a second launch and a clip alone give the same bits.  Returns the figures."""
    yd, Sd = dev(y), dev(S)
    sc, frames = Au.spectral_convergence(yd, Sd, n_fft, hop, per_frame=True)
    assert sc.dtype == torch.float64 and tuple(sc.shape) == (len(y),) and frames.dtype == torch.float64 and tuple(frames.shape) == (*S.shape[:2], 2)
    sc2, frames2 = Au.spectral_convergence(yd, Sd, n_fft, hop, per_frame=True)
    assert torch.equal(sc.view(torch.int64), sc2.view(torch.int64)) and torch.equal(frames.view(torch.int64), frames2.view(torch.int64))
    clips = torch.empty(len(y), 2, dtype=torch.float64, device=DEV)
    _lib.call("nsg_audio_spectral_convergence", _p(yd), _p(Sd), _p(None), _p(clips), *S.shape[:2], n_fft, hop, _stream())      # frame_sums NULL
    got, fr = sc.cpu().numpy(), frames.cpu().numpy()
    assert np.array_equal(R.figure(clips.cpu().numpy()), got), tag
    for b in range(len(y)):
        s64 = R.convergence_sums(y[b].astype(np.float64), S[b].T.astype(np.float64), n_fft, hop)
        sc64 = float(R.figure(s64.sum(0)))
        bound = R.sc_eps(n_fft) * (1.0 + sc64)
        print(f"[{tag}] clip {b}: sc={got[b]:.6e} sc64={sc64:.6e} |diff|={abs(got[b] - sc64):.2e} bound={bound:.2e} share={abs(got[b] - sc64) / bound:.3f}")
        assert abs(got[b] - sc64) <= bound, (tag, b)
        assert np.allclose(fr[b, :, 1], s64[:, 1], rtol=1e-14, atol=0)    # the same fp32 numbers squared and summed in fp64, in another order
        tot = np.array([math.fsum(fr[b, :, 0]), math.fsum(fr[b, :, 1])])  # exact; the device's tree over T <= 24 frames is 5 adds deep: 5.5e-16
        assert np.allclose(tot, clips[b].cpu().numpy(), rtol=1e-15, atol=0), (tag, b)
        one = Au.spectral_convergence(yd[b:b + 1].contiguous(), Sd[b:b + 1].contiguous(), n_fft, hop)
        assert one.view(torch.int64).item() == sc[b].view(torch.int64).item(), (tag, b)
    return got


@pytest.mark.parametrize("n_fft,hop,T", R.GL_FAST_CASES)
def test_spectral_convergence_of_a_griffin_lim_output(n_fft, hop, T):
    """gl_case magnitudes with the kernels' own fast Griffin-Lim output for them (the short grid 512/128 T=2 among them)."""
    S, u = E.gl_case(n_fft, hop, T)
    y = Au.griffin_lim(dev(S), n_fft, hop, 3, dev(u), momentum=0.99).cpu().numpy()
    check_convergence(y, S, n_fft, hop, f"sc gl {n_fft}/{hop} T={T}")


@pytest.mark.parametrize("n_fft,hop,T", [(512, 128, 24), (1024, 256, 24), (2048, 512, 9)])
def test_spectral_convergence_of_a_signal_with_its_own_magnitudes(n_fft, hop, T):
    """S = |stft64(y)| of a band-limited signal: the true figure is the rounding of S (below 2^-24), and the device's is at most eps."""
    y, S = R.band_limited_case(n_fft, hop, T)
    got = check_convergence(y[None], S.T[None], n_fft, hop, f"sc band-limited {n_fft}/{hop} T={T}")
    assert got[0] <= R.sc_eps(n_fft)


def test_spectral_convergence_of_zero_magnitudes():
    y, S = R.band_limited_case(512, 128, 9)
    yd = dev(np.stack([np.zeros_like(y), y, y]))
    Sd = dev(np.stack([np.zeros_like(S.T), np.zeros_like(S.T), S.T]))
    sc = Au.spectral_convergence(yd, Sd, 512, 128).cpu().numpy()
    assert sc[0] == 0.0 and sc[1] == float("inf") and 0.0 < sc[2] <= R.sc_eps(512)


# ----------------------------------------------------------------------------------------------------------------------
# wiring
# ----------------------------------------------------------------------------------------------------------------------
def test_inv_mel_spectrogram_with_momentum_is_its_pieces():
    rs = np.random.RandomState(5)
    mel = dev(rs.rand(2, 80, 12).astype(np.float32))
    a0 = dev(rs.rand(2, 12, 513).astype(np.float32))
    got = Au.inv_mel_spectrogram(mel, iters=5, angles0=a0, momentum=0.99)
    want = Au.inv_preemphasis(Au.griffin_lim(Au.mel_to_linear(mel), 1024, 256, 5, a0, momentum=0.99))
    assert torch.equal(got, want)
    plain = Au.inv_mel_spectrogram(mel, iters=5, angles0=a0)
    assert torch.equal(plain, Au.inv_preemphasis(Au.griffin_lim(Au.mel_to_linear(mel), 1024, 256, 5, a0))) and not torch.equal(plain, got)
    one = Au.inv_mel_spectrogram(mel[0].cpu().numpy(), iters=5, angles0=a0[:1].cpu().numpy(), momentum=0.99)
    assert np.array_equal(one, got[0].cpu().numpy())


def _pooled(model, loader, angles, iters, momentum):
    """test_conversion_f0's figures from the pieces (tests/test_gpu_f0_stats.py's pooling), with the inversion at `momentum`."""
    from tests.test_gpu_f0_stats import HOP
    stats, sc = np.zeros(10), []
    for (ws, ls, wt, lt, g), a0 in zip(loader, angles):
        ws, wt = ws.to(DEV), wt.to(DEV)
        mel_s, mel_t = Au.melspectrogram(ws, lengths=ls), Au.melspectrogram(wt, lengths=lt)
        fs, ft = 1 + ls.numpy() // HOP, 1 + lt.numpy() // HOP
        Tc = mel_s.shape[2] // 4 * 4
        fc = np.minimum(fs, Tc) // 4 * 4
        _, conv = evaluate.convert_voice(model, mel_s[:, :, :Tc].contiguous(), g)
        S = Au.mel_to_linear(conv.squeeze(1).contiguous())
        y = Au.griffin_lim(S, 1024, HOP, iters, a0, momentum=momentum)
        sc += Au.spectral_convergence(y, S, 1024, HOP).tolist()
        wav_c = Au.inv_mel_spectrogram(conv.squeeze(1), iters=iters, angles0=a0, momentum=momentum)
        assert torch.equal(wav_c, Au.inv_preemphasis(y))
        f0_c, f0_t = Au.f0(wav_c, lengths=HOP * (fc - 1))[0], Au.f0(wt, lengths=lt)[0]
        cost, steps, path = Au.dtw(Au.mel_cepstra(conv, fc), Au.mel_cepstra(mel_t, ft), fc, ft, want_path=True)
        stats += Au.f0_distortion(f0_c, f0_t, path, steps)[3].sum(0).cpu().numpy()
    return stats, sc


def test_test_conversion_f0_with_momentum_is_pooled_from_the_pieces(capsys):
    from tests.test_gpu_f0_stats import HOP, pair_batch
    torch.manual_seed(13)
    model = models.VQVAE(1, 16, 32, n_speakers=2).to(DEV).eval()
    loader = [pair_batch(1, 10240, 11000), pair_batch(2, 9000, 8200)]
    gen = torch.Generator().manual_seed(4)
    angles = [torch.rand(2, (1 + b[0].shape[1] // HOP) // 4 * 4, 513, generator=gen).to(DEV) for b in loader]
    iters = 4
    for momentum in (0.99, 0.0):
        got = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=iters, angles0=angles, momentum=momentum)
        assert "spectral convergence" in capsys.readouterr().out and got["clips"] == 4
        stats, sc = _pooled(model, loader, angles, iters, momentum)
        fig = got["converted"]
        assert np.array_equal(np.asarray(fig["stats"][:4]), stats[:4]) and np.allclose(fig["stats"], stats, rtol=1e-13, atol=0)
        assert len(sc) == 4 and fig["spectral_convergence"] == pytest.approx(np.mean(sc), rel=1e-12) and 0.0 < fig["spectral_convergence"] < 2.0
        assert "spectral_convergence" not in got["source"]
        if momentum == 0.0:                    # the default is the code path there was: inv_mel_spectrogram's plain call, bit for bit
            plain = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=iters, angles0=angles)
            assert plain == got or str(plain) == str(got)                  # (as text: a NaN figure equals itself)
            assert np.array_equal(np.asarray(fig["stats"]), np.asarray(plain["converted"]["stats"]))
