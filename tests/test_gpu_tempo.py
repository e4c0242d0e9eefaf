"""GPU: nsg_audio_tempo equals the fp32 restatement of its contract (tests/helpers/tempo_ref.py: wsola_f32) bit for bit -- the
positions exactly, the output by bit pattern, the rows' padding included -- across the envelope: the smallest and the largest
sizes, an odd overlap and a search width that is no multiple of a lane's run, every search width class (a lane's run of 2, 4 and
8 candidates) with every overlap mod 4, an overlap as long as the hop, a search of one position, the factors 0.25 .. 4, ragged lengths down to none, a clip
alone and as a row of a larger batch.  Inputs and outputs sit in guarded buffers, with NaN past each clip's length: a read past a
length or a row's end would reach the result, a store outside the outputs would reach the guards.  Then audio.tempo,
audio.pitch_shift, audio.random_augment and preprocess's augmented copies end to end."""
import os

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, ops, preprocess
from neural_sound_generation_amd.ops import _p, _stream
from tests.helpers import tempo_ref as R

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)
DEV = torch.device("cuda:0")
GUARD = 67
SENTINEL = 0x7F7F7F7F
SR = 22050
FACTORS = [0.25, 0.85, 1.0, 1.15, 4.0]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def clip(L, seed, f0=140.0):
    """A gliding six-harmonic tone with some noise, a stretch of noise alone: similar and dissimilar candidates."""
    rs = np.random.RandomState(seed)
    n = np.arange(L, dtype=np.float64)
    phase = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.3 * n / max(L, 1)) / SR)
    x = sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7)) + 0.05 * rs.standard_normal(L)
    a, b = int(0.6 * L), int(0.8 * L)
    x[a:b] = 0.3 * rs.standard_normal(b - a)
    return x.astype(np.float32)


def launch(host, factors, S, O, W, lengths=None, L_out=None):
    """nsg_audio_tempo on host (B, L) in guarded buffers (NaN past each length too) -> (out (B, L_out), positions (B, M_max),
    out_lengths), the guards checked."""
    B, L = host.shape
    host = host.copy()
    lens = np.full(B, L, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    for b in range(B):
        host[b, lens[b]:] = np.nan
    f = np.array(np.broadcast_to(np.asarray(factors, dtype=np.float64), (B,)))
    out_lens = ops.tempo_out_lengths(lens, f)
    L_out = max(1, int(out_lens.max())) if L_out is None else L_out
    M_max = -(-L_out // (S - O))
    buf = torch.full((host.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    wav = buf[GUARD:GUARD + host.size].view(B, L)
    wav.copy_(torch.from_numpy(host))
    obuf = torch.full((B * L_out + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    pbuf = torch.full((B * M_max + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    out, pos = obuf[GUARD:GUARD + B * L_out], pbuf[GUARD:GUARD + B * M_max]
    lens_d = None if lengths is None else torch.from_numpy(lens.astype(np.int32)).to(DEV)
    f_d, ol_d = torch.from_numpy(f).to(DEV), torch.from_numpy(out_lens.astype(np.int32)).to(DEV)
    _lib.call("nsg_audio_tempo", _p(wav), _p(lens_d), _p(f_d), _p(ol_d), _p(out), _p(pos), B, L, L_out, S, O, W, None, 0, _stream())
    whole, pwhole = obuf.cpu().numpy(), pbuf.cpu().numpy()
    assert np.isnan(whole[:GUARD]).all() and np.isnan(whole[GUARD + B * L_out:]).all(), "a store outside out"
    assert (pwhole[:GUARD] == SENTINEL).all() and (pwhole[GUARD + B * M_max:] == SENTINEL).all(), "a store outside positions"
    return whole[GUARD:GUARD + B * L_out].reshape(B, L_out), pwhole[GUARD:GUARD + B * M_max].reshape(B, M_max), out_lens


def check(host, factors, S, O, W, lengths=None, L_out=None):
    out, pos, out_lens = launch(host, factors, S, O, W, lengths, L_out)
    B = host.shape[0]
    f = np.broadcast_to(np.asarray(factors, dtype=np.float64), (B,))
    assert np.isfinite(out).all(), "an element was not written, or a NaN was read"
    assert (pos != SENTINEL).all(), "a position was not written"
    for b in range(B):
        n = None if lengths is None else lengths[b]
        want, want_len, want_q = R.wsola_f32(host[b], n, f[b], S, O, W, L_out=out.shape[1])
        assert want_len == out_lens[b]
        assert np.array_equal(pos[b], want_q), (b, np.flatnonzero(pos[b] != want_q)[:4].tolist(), pos[b][:6], want_q[:6])
        bad = bits(out[b]) != bits(want)
        assert not bad.any(), (b, int(bad.sum()), np.flatnonzero(bad)[:4].tolist(), out[b][bad][:4], want[bad][:4])
    return out, pos, out_lens


CASES = {                                   # name: (L, S, O, W)
    "smallest": (700, 16, 4, 8),
    "small": (1500, 64, 8, 20),
    "odd_overlap_and_width": (900, 32, 7, 5),
    "all_blend": (500, 16, 8, 6),
    "no_search": (900, 32, 8, 1),
    "run_of_4": (4000, 256, 33, 700),
    "run_of_8": (5000, 300, 30, 1100),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement(name):
    L, S, O, W = CASES[name]
    host = np.stack([clip(L, 10 * len(name) + b, f0=120.0 + 40.0 * b) for b in range(len(FACTORS))])
    out, pos, out_lens = check(host, FACTORS, S, O, W)
    assert out_lens.tolist() == [4 * L, int(np.floor(L / 0.85)), L, int(np.floor(L / 1.15)), L // 4]
    assert np.array_equal(bits(out[2, :L]), bits(host[2]))                                  # factor 1
    if W > 1:
        assert len(np.unique((pos[1, 1:] - np.floor(np.arange(1, pos.shape[1]) * (S - O) * 0.85))[pos[1, 1:] >= 0])) > 1   # the search moved


@pytest.mark.parametrize("O", [4, 5, 6, 7])
@pytest.mark.parametrize("W", [20, 513, 1025])
def test_every_run_with_every_tail_of_the_overlap(W, O):
    """The search is one template over (a lane's run, O mod 4): W = 20, 513, 1025 are runs of 2, 4 and 8 candidates, O = 4 .. 7 the
    four remainders, so each of the twelve instantiations runs here."""
    host = np.stack([clip(2500, 7 * W + O + b, f0=110.0 + 35.0 * b) for b in range(len(FACTORS))])
    check(host, FACTORS, 64, O, W)


def test_the_defaults_on_a_second_of_audio():
    host = np.stack([clip(SR, 3), clip(SR, 4, f0=210.0)])
    out, pos, out_lens = check(host, [0.85, 1.15], *audio.tempo_sizes(SR))
    assert out_lens.tolist() == [25941, 19173]


def test_the_corner_of_the_envelope():
    host = np.stack([clip(30000, 5), clip(30000, 6, f0=90.0)])
    check(host, [0.85, 1.15], 8192, 2048, 2048)


def test_ragged_lengths_and_per_clip_factors_in_one_launch():
    S, O, W, L = 64, 8, 20, 1200
    lengths = [0, 1, 56, 63, L, 777, 3]
    factors = [1.0, 0.25, 0.85, 1.15, 0.85, 1.15, 4.0]
    host = np.stack([clip(L, 40 + b, f0=100.0 + 30.0 * b) for b in range(len(lengths))])
    out, pos, out_lens = check(host, factors, S, O, W, lengths)
    assert out_lens.tolist() == [0, 4, 65, 54, 1411, 675, 0]
    for b, n in enumerate(out_lens):
        assert (bits(out[b, n:]) == 0).all() and (pos[b, -(-n // 56):] == -1).all() and (pos[b, :-(-n // 56)] >= 0).all()


def test_a_clip_alone_and_as_a_row_of_a_larger_batch():
    S, O, W, n = 64, 8, 20, 1900
    x = clip(n, 7, f0=180.0)
    alone, alone_q, alone_len = check(x[None], 0.85, S, O, W)
    batch = np.stack([clip(3000, 50 + b) for b in range(5)])
    batch[3, :n] = x
    out, pos, out_lens = check(batch, [1.15, 0.25, 1.0, 0.85, 4.0], S, O, W, [3000, 2500, 700, n, 3000])
    m = alone_len[0]
    assert out_lens[3] == m and np.array_equal(bits(out[3, :m]), bits(alone[0])) and np.array_equal(pos[3, :alone_q.shape[1]], alone_q[0])


def test_identity_and_periodic_continuation_on_the_device():
    x = np.random.RandomState(0).standard_normal(5000).astype(np.float32)
    out, pos, _ = launch(x[None], 1.0, 64, 8, 20)
    assert np.array_equal(bits(out[0]), bits(x)) and np.array_equal(pos[0], np.arange(pos.shape[1]) * 56)
    period = np.random.RandomState(1).randint(-8, 9, 37).astype(np.float32)
    x = np.tile(period, 200)[:6000]
    factors = [0.8, 0.85, 1.15, 1.25]
    out, pos, out_lens = launch(np.stack([x] * 4), factors, 128, 16, 48)
    for b, n in enumerate(out_lens):
        assert n == R.out_length(6000, factors[b])
        assert np.array_equal(bits(out[b, :n - 200]), bits(np.tile(period, 400)[:n - 200])), factors[b]


def test_two_launches_give_the_same_bits_and_the_workspace_path_too():
    host = np.stack([clip(3000, 90 + b) for b in range(3)])
    a, b = launch(host, [0.85, 1.0, 1.15], 64, 8, 20), launch(host, [0.85, 1.0, 1.15], 64, 8, 20)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    wav = torch.from_numpy(host).to(DEV)
    out, out_lens = ops.tempo(wav, [0.85, 1.0, 1.15], 64, 8, 20)                              # without positions: they live in the workspace
    assert np.array_equal(bits(out.cpu().numpy()), bits(a[0])) and out_lens.dtype == np.int32 and np.array_equal(out_lens, a[2])
    out2, _, pos = ops.tempo(wav, [0.85, 1.0, 1.15], 64, 8, 20, want_positions=True)
    assert torch.equal(out, out2) and np.array_equal(pos.cpu().numpy(), a[1])


def tone(seconds=2.0, freq=140.3):
    n = np.arange(int(seconds * SR), dtype=np.float64)
    return sum(0.6 ** h * np.sin(2 * np.pi * freq * h * n / SR) for h in range(1, 7)).astype(np.float32)


def peak_hz(y, start, window, lo=60.0, hi=260.0):
    nfft = 1 << 18
    sp = np.abs(np.fft.rfft(np.asarray(y[start:start + window], dtype=np.float64) * np.hanning(window), nfft))
    a, b = int(lo * nfft / SR), int(hi * nfft / SR)
    return (a + int(np.argmax(sp[a:b]))) * SR / nfft


@pytest.mark.parametrize("factor,length", [(0.85, 51882), (1.15, 38347)])
def test_audio_tempo_keeps_the_pitch_of_a_tone(factor, length):
    x = tone()
    y, q = audio.tempo(x, factor, detail=True)
    want, _, want_q = R.wsola_f32(x, None, factor)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and len(y) == length
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(q, want_q)
    f = peak_hz(y, 8192, 16384, lo=100.0)
    print(f"factor {factor}: peak {f:.3f} Hz")
    assert abs(f - 140.3) < 0.25
    batch, lens = audio.tempo(torch.from_numpy(np.stack([x, x])).to(DEV), [factor, 1.0], lengths=[len(x), 30000])
    assert lens.tolist() == [length, 30000] and tuple(batch.shape) == (2, max(length, 30000))
    assert np.array_equal(bits(batch[0, :length].cpu().numpy()), bits(want)) and torch.equal(batch[1, :30000].cpu(), torch.from_numpy(x[:30000]))
    assert not batch[1, 30000:].any()


@pytest.mark.parametrize("num,den", [(196, 185), (185, 196), (3, 2), (2, 3)])
def test_audio_pitch_shift_moves_the_pitch_of_a_tone(num, den):
    x = tone()
    y = audio.pitch_shift(x, num, den)
    assert isinstance(y, np.ndarray) and len(y) == len(x)
    f = peak_hz(y, 8192, 8192)
    print(f"{num} / {den}: peak {f:.3f} Hz, want {140.3 * num / den:.3f}")
    assert abs(f - 140.3 * num / den) < 0.25
    if num == 3:
        yb, lens = audio.pitch_shift(torch.from_numpy(np.stack([x, x])).to(DEV), num, den, lengths=[len(x), 20000])
        assert lens.tolist() == [len(x), 20000] and np.array_equal(bits(yb[0].cpu().numpy()[:len(x)]), bits(y))


def test_random_augment_reproduces_from_a_seed():
    host = np.stack([clip(6000, 20 + b) for b in range(3)])
    wav = torch.from_numpy(host).to(DEV)
    noise = np.random.RandomState(3).standard_normal(2500).astype(np.float32)
    runs = [audio.random_augment(wav, [6000, 4000, 5000], torch.Generator().manual_seed(11), noise=noise) for _ in range(2)]
    (a, la, pa), (b, lb, pb) = runs
    assert torch.equal(a, b) and np.array_equal(la, lb) and all(np.array_equal(pa[k], pb[k]) for k in pa)
    assert la.tolist() == ops.tempo_out_lengths([6000, 4000, 5000], pa["tempo"]).tolist() and tuple(a.shape) == (3, int(la.max()))
    mid, _ = audio.tempo(wav, pa["tempo"], lengths=[6000, 4000, 5000])
    gain = (10.0 ** (pa["gain_db"] / 20.0)).astype(np.float32)
    for r in range(3):                                                                      # the mix is the restatement's, on the tempo's output
        want = R.mix_f32(mid[r].cpu().numpy(), la[r], noise, gain[r], pa["level"][r], pa["offset"][r])[0]
        assert np.array_equal(bits(a[r].cpu().numpy()), bits(want))
    c, lc, pc = audio.random_augment(wav, None, torch.Generator().manual_seed(12))             # another seed, no noise: the gain alone
    assert not np.array_equal(pc["tempo"], pa["tempo"][:3]) and set(pc) == {"tempo", "gain_db"}
    mid, _ = audio.tempo(wav, pc["tempo"])
    g = torch.from_numpy((10.0 ** (pc["gain_db"] / 20.0)).astype(np.float32)).to(DEV)[:, None]
    assert torch.equal(c, g * mid + 0.0)


def test_process_utterances_writes_augmented_copies(tmp_path):
    rs = np.random.RandomState(5)
    clips = [0.5 * clip(int(SR * rs.uniform(0.3, 0.6)), 60 + i, f0=110.0 + 25.0 * i) for i in range(5)]
    texts, speakers = ["utterance %d" % i for i in range(5)], [3, 1, 4, 1, 5]
    noise = (0.1 * rs.standard_normal(9000)).astype(np.float32)
    plain = preprocess.process_utterances(clips, texts, str(tmp_path / "plain"), "t", 7, speakers)
    outs = {}
    for bc in (64, 2):
        outs[bc] = preprocess.process_utterances(clips, texts, str(tmp_path / ("aug%d" % bc)), "t", 7, speakers, batch_clips=bc, augment_copies=2,
                                                 augment_seed=9, noise=noise)
    meta = outs[64]
    assert meta == outs[2] and meta[:5] == plain and len(meta) == 15
    params = audio.augment_draws(10, torch.Generator().manual_seed(9), noise_len=9000)
    for k, row in enumerate(meta):
        c, i = divmod(k, 5)
        assert row[0] == "t-audio-%05d.npy" % (7 + c * 5 + i) and row[1] == "t-mel-%05d.npy" % (7 + c * 5 + i) and row[3:] == (texts[i], speakers[i])
        files = [np.load(os.path.join(str(tmp_path / d), row[j])) for d in ("aug64", "aug2") for j in (0, 1)]
        assert np.array_equal(files[0], files[2]) and np.array_equal(files[1], files[3])    # the files do not depend on batch_clips
        if c == 0:
            assert np.array_equal(files[0], np.load(os.path.join(str(tmp_path / "plain"), row[0])))
            assert np.array_equal(files[1], np.load(os.path.join(str(tmp_path / "plain"), row[1])))
        else:                                                                               # the copy's duration follows its drawn tempo
            n = R.out_length(len(clips[i]), params["tempo"][(c - 1) * 5 + i])
            assert row[2] == (1 + n // 256) * 256 and files[1].shape == (1 + n // 256, 80)
            assert abs(float(np.abs(files[0]).max()) - 0.999) < 1e-6
    with pytest.raises(ValueError, match="augment_copies"):
        preprocess.process_utterances(clips, texts, str(tmp_path / "bad"), augment_copies=-1)
