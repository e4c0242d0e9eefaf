"""GPU: nsg_f0_viterbi equals the fp32 restatement of its contract (tests/helpers/f0_track_ref.py: viterbi_f32) bit for bit --
state, cost, f0 and ap -- on random candidate tensors with random counts, at clip lengths around the staging chunk of 64 frames
and just past the 2 048 frames whose back-pointers LDS holds, on the hand-built tie cases, with counts outside [0, 8], NaN in the
slots past a count, ragged frame counts and a clip alone against a row of a batch; then audio.f0_track end to end on the prototype
signal, and evaluate.test_conversion_f0(tracker="viterbi") against figures pooled by hand.  Inputs carry NaN where the kernel must
not read; outputs sit in guarded buffers."""
import json

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, evaluate, models, ops
from tests.helpers import f0_ref as R
from tests.helpers import f0_track_ref as K

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)
DEV = torch.device("cuda:0")
GUARD = 67
NC = 8
HOP = 256
COSTS = dict(logf_top=8.9, octave_cost=0.01, jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3)
COST_ORDER = ("logf_top", "octave_cost", "jump_cost", "vuv_cost", "unvoiced_cost")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def random_candidates(rs, B, T, walk=True):
    """Candidate tensors like a tracker's: log-frequencies 6 .. 8.9 by descending frequency, d' in (0, 1), counts 0 .. 8; NaN in
    every slot past a count."""
    count = rs.randint(0, NC + 1, (B, T)).astype(np.int32)
    logf = -np.sort(-rs.uniform(6.0, 8.9, (B, T, NC)), axis=2).astype(np.float32)
    ap = rs.uniform(0.0, 1.0, (B, T, NC)).astype(np.float32)
    if walk:                                           # one slot a frame follows a slow track with a low d', so paths stay voiced for stretches
        track = 7.0 + np.cumsum(rs.normal(0, 0.01, (B, T)), axis=1)
        logf[:, :, 2] = track
        ap[:, :, 2] = rs.uniform(0.0, 0.2, (B, T))
    f0 = np.exp2(logf.astype(np.float64)).astype(np.float32)
    past = np.arange(NC)[None, None, :] >= count[:, :, None]
    for a in (logf, ap, f0):
        a[past] = np.nan
    return logf, ap, f0, count


def launch(logf, ap, f0, count, frames=None, costs=COSTS):
    """ops.f0_viterbi on host tensors (B, T, 8) / (B, T) with outputs in guarded buffers -> (state, cost, f0, ap) numpy."""
    B, T = count.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (logf, ap, f0, count)]
    fbuf = torch.full((2, B * T + 2 * GUARD), float("nan"), dtype=torch.float32, device=DEV)
    sbuf = torch.full((B * T + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    cbuf = torch.full((B + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    out = (sbuf[GUARD:GUARD + B * T].view(B, T), cbuf[GUARD:GUARD + B], fbuf[0, GUARD:GUARD + B * T].view(B, T), fbuf[1, GUARD:GUARD + B * T].view(B, T))
    got = ops.f0_viterbi(*dev, *(costs[k] for k in COST_ORDER), frames=frames, out=out)
    assert all(g is o for g, o in zip(got, out))
    fw, sw, cw = fbuf.cpu().numpy(), sbuf.cpu().numpy(), cbuf.cpu().numpy()
    assert np.isnan(fw[:, :GUARD]).all() and np.isnan(fw[:, GUARD + B * T:]).all(), "a store outside f0 / ap"
    assert (sw[:GUARD] == -77).all() and (sw[GUARD + B * T:] == -77).all(), "a store outside state"
    assert np.isnan(cw[:GUARD]).all() and np.isnan(cw[GUARD + B:]).all(), "a store outside cost"
    return (sw[GUARD:GUARD + B * T].reshape(B, T), cw[GUARD:GUARD + B], fw[0, GUARD:GUARD + B * T].reshape(B, T),
            fw[1, GUARD:GUARD + B * T].reshape(B, T))


def check(logf, ap, f0, count, frames=None, costs=COSTS):
    state, cost, f, a = launch(logf, ap, f0, count, frames, costs)
    assert np.isfinite(f).all() and np.isfinite(a).all() and np.isfinite(cost).all() and (state != -77).all(), "an element was not written, or a NaN was read"
    for b in range(count.shape[0]):
        ws, wc, wf, wa = K.viterbi_f32(logf[b], ap[b], f0[b], count[b], None if frames is None else frames[b], **costs)
        assert np.array_equal(state[b], ws), (b, np.flatnonzero(state[b] != ws)[:6].tolist(), state[b][state[b] != ws][:6], ws[state[b] != ws][:6])
        assert bits(cost[b]) == bits(wc), (b, cost[b], wc)
        assert np.array_equal(bits(f[b]), bits(wf)) and np.array_equal(bits(a[b]), bits(wa)), b
    return state, cost, f, a


LDS = ops.F0_VITERBI_LDS_FRAMES


@pytest.mark.parametrize("Tb", [0, 1, 2, 63, 64, 65, 300])
def test_kernel_equals_the_restatement(Tb):
    rs = np.random.RandomState(100 + Tb)
    B, T = 2, max(Tb, 1) + 3
    state, cost, f, a = check(*random_candidates(rs, B, T), frames=[Tb, Tb])
    assert (state[:, Tb:] == -1).all() and (bits(f[:, Tb:]) == 0).all() and (a[:, Tb:] == 1.0).all()
    if Tb >= 63:
        assert (state[:, :Tb] > 0).any() and (state[:, :Tb] == 0).any()      # voiced and unvoiced stretches
    if Tb == 0:
        assert (bits(cost) == 0).all()


def test_just_past_the_frames_lds_holds():
    """T = 2 049: the back-pointers go to the workspace, and the back-trace takes two blocks (frame 2 048 alone, then 0 .. 2 047); a
    second clip ends inside the first block; and T = 2 048, the last that needs no workspace."""
    rs = np.random.RandomState(7)
    assert _lib.query("nsg_f0_viterbi_workspace_bytes", 2, LDS + 1) > 0 and _lib.query("nsg_f0_viterbi_workspace_bytes", 2, LDS) == 0
    state, _, _, _ = check(*random_candidates(rs, 2, LDS + 1), frames=[LDS + 1, 1000])
    assert (state[0] >= 0).all() and (state[1, 1000:] == -1).all()
    check(*random_candidates(rs, 1, LDS))


def test_a_workspace_that_is_too_small_is_refused():
    B, T = 2, LDS + 1
    z = torch.zeros(B, T, NC, device=DEV)
    cnt, st = torch.zeros(B, T, dtype=torch.int32, device=DEV), torch.full((B, T), -77, dtype=torch.int32, device=DEV)
    cost, f, a = torch.zeros(B, device=DEV), torch.zeros(B, T, device=DEV), torch.zeros(B, T, device=DEV)
    need = _lib.query("nsg_f0_viterbi_workspace_bytes", B, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = ops._p
    with pytest.raises(_lib.NsgError, match="nsg_f0_viterbi: workspace too small"):
        _lib.call("nsg_f0_viterbi", p(z), p(z), p(z), p(cnt), None, p(st), p(cost), p(f), p(a), B, T, 8.9, 0.01, 0.35, 0.14, 0.3, p(ws), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert (st == -77).all()                            # nothing was launched


@pytest.mark.parametrize("name", sorted(K.hand_cases()))
def test_hand_built_paths(name):
    logf, ap, f0, count, frames, costs, states, cost = K.hand_cases()[name]
    got = check(logf[None], ap[None], f0[None], count[None], None if frames is None else [frames], costs)
    assert got[0][0].tolist() == states and float(got[1][0]) == cost


def test_counts_outside_the_range_are_clamped_and_slots_past_a_count_are_not_read():
    rs = np.random.RandomState(11)
    logf, ap, f0, count = random_candidates(rs, 2, 40)
    want = launch(logf, ap, f0, count)
    wide = count.copy()
    wide[count == NC] = 11
    wide[count == 0] = -3
    assert (wide == 11).any() and (wide == -3).any()
    got = check(logf, ap, f0, wide)
    clean = [np.nan_to_num(a, nan=0.5) for a in (logf, ap, f0)]              # the same tensors with numbers where the NaN were
    for g, w, c in zip(got, want, launch(*clean, count)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)) and np.array_equal(c.view(np.uint32), w.view(np.uint32))


def test_ragged_frames_in_one_launch_and_a_clip_alone_against_row_3():
    rs = np.random.RandomState(21)
    T = 150
    logf, ap, f0, count = random_candidates(rs, 5, T)
    frames = [T, 0, 64, 97, 1]
    state, cost, f, a = check(logf, ap, f0, count, frames)
    again = ops.f0_viterbi(*(torch.from_numpy(x).to(DEV) for x in (logf, ap, f0, count)), *(COSTS[k] for k in COST_ORDER),
                           frames=torch.tensor(frames, dtype=torch.int32, device=DEV))   # the same frame counts as a device tensor
    for g, w in zip(again, (state, cost, f, a)):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))
    alone = check(logf[3:4, :97], ap[3:4, :97], f0[3:4, :97], count[3:4, :97])
    assert np.array_equal(alone[0][0], state[3, :97]) and bits(alone[1][0]) == bits(cost[3])
    assert np.array_equal(bits(alone[2][0]), bits(f[3, :97])) and np.array_equal(bits(alone[3][0]), bits(a[3, :97]))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_f0_track_on_the_prototype_signal():
    x, truth_n, sr, W, hop, tau_min, tau_max = K.prototype_signal()
    fmin, fmax = 65.0, 490.0
    assert audio.f0_lags(sr, fmin, fmax) == (tau_min, tau_max)
    f, a, state, cost = audio.f0_track(x, fmin=fmin, fmax=fmax, detail=True)
    assert all(isinstance(v, np.ndarray) for v in (f, a, state, cost)) and f.shape == a.shape == state.shape == (138,) and state.dtype == np.int32
    cf, ca, cl, cnt = audio.f0_candidates(x, fmin=fmin, fmax=fmax)
    ws, wc, wf, wa = K.viterbi_f32(cl, ca, cf, cnt, None, np.log2(sr / tau_min), 0.01, 0.35, 0.14, 0.3)
    assert np.array_equal(state, ws) and bits(cost) == bits(wc) and np.array_equal(bits(f), bits(wf)) and np.array_equal(bits(a), bits(wa))
    f2, a2 = audio.f0_track(x, fmin=fmin, fmax=fmax)
    assert np.array_equal(bits(f2), bits(f)) and np.array_equal(bits(a2), bits(a))
    voiced, tail = K.prototype_frames(len(x), sr, W, hop)
    truth = truth_n[np.minimum(np.arange(len(voiced)) * hop, len(x) - 1)]
    for uc in (0.3, 0.2, 0.45):
        fu, _ = audio.f0_track(x, fmin=fmin, fmax=fmax, unvoiced_cost=uc)
        on = fu > 0
        off = np.abs(1200.0 * np.log2(np.where(on, fu, truth).astype(np.float64) / truth))
        assert not (voiced & on & (off > 50.0)).any() and not (voiced & ~on).any() and not (tail & on).any(), uc
    raw, _ = audio.f0(x, fmin=fmin, fmax=fmax)
    on = raw > 0
    off = np.abs(1200.0 * np.log2(np.where(on, raw, truth).astype(np.float64) / truth))
    assert (voiced & on & (off > 50.0)).any() and (voiced & ~on).any()       # what the tracker repairs
    # a batch with lengths: the clip's frames are what they are alone; the frames past it are (0, 1, -1)
    n = 20000
    batch = torch.from_numpy(np.stack([x, x])).to(DEV)
    bf, ba, bs, bc = audio.f0_track(batch, fmin=fmin, fmax=fmax, lengths=[len(x), n], detail=True)
    assert torch.equal(bf[0], torch.from_numpy(f).to(DEV)) and torch.equal(bs[0], torch.from_numpy(state).to(DEV))
    sf, sa, ss, sc = audio.f0_track(x[:n], fmin=fmin, fmax=fmax, detail=True)
    nb = 1 + n // hop
    assert np.array_equal(bits(bf[1, :nb].cpu().numpy()), bits(sf)) and np.array_equal(bs[1, :nb].cpu().numpy(), ss)
    assert (bs[1, nb:] == -1).all() and not bf[1, nb:].any() and (ba[1, nb:] == 1).all() and bits(bc[1].cpu().numpy()) == bits(sc)


def harmonic(freq_of_n, L, sr=22050):
    phase = 2 * np.pi * np.cumsum(freq_of_n(np.arange(L, dtype=np.float64)) / sr)
    return sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7)).astype(np.float32)


def pair_batch(seed, L_src, L_tgt):
    """Two clips a side: gliding harmonic tones with a quiet tail, so that frames are voiced and unvoiced."""
    rs = np.random.RandomState(seed)

    def side(L, lens, base):
        w = np.zeros((2, L), dtype=np.float32)
        for b, n in enumerate(lens):
            w[b, :n] = harmonic(lambda m, f=base * (1 + 0.2 * b): f * (1.0 + 0.2 * m / n), n)
            w[b, int(0.8 * n):n] = 0.02 * rs.standard_normal(n - int(0.8 * n))
        return torch.from_numpy(0.3 * w), torch.tensor(lens)
    ws, ls = side(L_src, [L_src, L_src - 1500], 120.0)
    wt, lt = side(L_tgt, [L_tgt - 900, L_tgt], 170.0)
    return ws, ls, wt, lt, torch.from_numpy(rs.randint(0, 2, 2).astype(np.int64))


def test_test_conversion_f0_with_the_viterbi_tracker_is_pooled_from_the_pieces():
    torch.manual_seed(13)
    model = models.VQVAE(1, 16, 32, n_speakers=2).to(DEV).eval()
    loader = [pair_batch(1, 10240, 11000), pair_batch(2, 9000, 8200)]
    gen = torch.Generator().manual_seed(4)
    angles = [torch.rand(2, (1 + b[0].shape[1] // HOP) // 4 * 4, 513, generator=gen).to(DEV) for b in loader]
    iters = 4
    options = dict(jump_cost=0.5, unvoiced_cost=0.35)
    got = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=iters, angles0=angles, tracker="viterbi", tracker_options=options)
    plain = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=iters, angles0=angles)
    yin = evaluate.test_conversion_f0(None, model, loader, DEV, 0, iters=iters, angles0=angles, tracker="yin")
    assert json.dumps(yin) == json.dumps(plain)         # (as text: a NaN figure equals itself)
    assert got["clips"] == 4

    pooled = {"converted": np.zeros(10), "source": np.zeros(10)}
    mcds = {"converted": [], "source": []}
    for (ws, ls, wt, lt, g), a0 in zip(loader, angles):
        ws, wt = ws.to(DEV), wt.to(DEV)
        mel_s, mel_t = audio.melspectrogram(ws, lengths=ls), audio.melspectrogram(wt, lengths=lt)
        fs, ft = 1 + ls.numpy() // HOP, 1 + lt.numpy() // HOP
        Tc = mel_s.shape[2] // 4 * 4
        fc = np.minimum(fs, Tc) // 4 * 4
        _, conv = evaluate.convert_voice(model, mel_s[:, :, :Tc].contiguous(), g)
        wav_c = audio.inv_mel_spectrogram(conv.squeeze(1), iters=iters, angles0=a0)
        f0_t, _ = audio.f0_track(wt, lengths=lt, **options)
        for name, mel, frames, f0_x in (("converted", conv, fc, audio.f0_track(wav_c, lengths=HOP * (fc - 1), **options)[0]),
                                        ("source", mel_s, fs, audio.f0_track(ws, lengths=ls, **options)[0])):
            cost, steps, path = audio.dtw(audio.mel_cepstra(mel, frames), audio.mel_cepstra(mel_t, ft), frames, ft, want_path=True)
            pooled[name] += audio.f0_distortion(f0_x, f0_t, path, steps)[3].sum(0).cpu().numpy()
            mcds[name] += ((cost / steps.float()) * audio.MCD_DB).double().tolist()
    for name in ("converted", "source"):
        st, fig = pooled[name], got[name]
        assert np.array_equal(np.asarray(fig["stats"][:4]), st[:4]) and np.allclose(fig["stats"], st, rtol=1e-13, atol=0)
        n, sdd = st[1], st[9]
        assert st[0] > 0 and fig["vuv_error"] == pytest.approx((st[2] + st[3]) / st[0], rel=1e-12)
        assert fig["mcd"] == pytest.approx(np.mean(mcds[name]), rel=1e-12) and fig["mcd"] == pytest.approx(plain[name]["mcd"], rel=1e-12)
        if n >= 2:
            assert fig["f0_rmse_cents"] == pytest.approx(1200.0 * np.sqrt(sdd / n), rel=1e-12)
    assert pooled["source"][1] >= 20


def test_test_conversion_f0_refuses_an_unknown_tracker_before_anything_is_launched():
    model = models.VQVAE(1, 16, 32, n_speakers=2).to(DEV)

    def loader():
        raise AssertionError("the loader was touched")
        yield

    with pytest.raises(ValueError, match="tracker must be"):
        evaluate.test_conversion_f0(None, model, loader(), DEV, 0, tracker="rapt")
