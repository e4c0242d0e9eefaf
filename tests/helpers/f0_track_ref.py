"""Host restatements of include/nsg.h's nsg_audio_f0_candidates and nsg_f0_viterbi (numpy only; no kernel, no torch).

  * candidates_f32(x, ...): the contract operation for operation in fp32 -- what the kernel must return bit for bit.  d' is
    f0_ref.yin_f32's own: that function hands a frame's d' to f0_ref._pick, and dprime_f32 / dprime_f64 run it (at a threshold
    that never matters) with _pick replaced for the call by a recorder, so nothing of the running sum is restated here.  The
    refinement is f0_ref._pick's too: a candidate lag tau is handed to it as the one lag "below the threshold".
  * candidates_f64(x, ...): the same definition on yin_f64's d'.
  * viterbi_f32(cand_logf, cand_ap, cand_f0, count, ...): every operation an np.float32 operation, in the contract's order: what
    the kernel must return bit for bit.  viterbi_f64: the same recurrence in fp64 -- the independent check of the path.

The candidate functions take one clip and return (cand_f0 (T, 8), cand_ap (T, 8), cand_logf (T, 8), count (T,) int32) for
T = 1 + L // hop frames; slots past count hold (0, 1, 0).  The viterbi functions take one clip's tensors (T, 8) / (T,) and the
number of frames that count, and return (state (T,) int32, cost, f0 (T,), ap (T,)); frames past that are (-1, 0, 1)."""
import numpy as np

from . import f0_ref as R

MAX_CANDIDATES = 8       # include/nsg.h: NSG_F0_MAX_CANDIDATES


def _dprime(yin, x, n, W, hop, tau_min, tau_max, sample_rate, L):
    """[T_b] rows d'(0 .. tau_max) exactly as `yin` (f0_ref.yin_f32 / yin_f64) forms them: recorded where it hands them to _pick."""
    rows = []
    pick = R._pick

    def record(dp, *rest):
        rows.append(dp.copy())
        return pick(dp, *rest)

    R._pick = record
    try:
        yin(x, n, W, hop, tau_min, tau_max, 0.5, sample_rate, L)
    finally:
        R._pick = pick
    return rows


def dprime_f32(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, sample_rate=22050.0, L=None):
    rows = _dprime(R.yin_f32, x, n, W, hop, tau_min, tau_max, sample_rate, L)
    assert all(r.dtype == np.float32 for r in rows)
    return rows


def dprime_f64(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, sample_rate=22050.0, L=None):
    return _dprime(R.yin_f64, x, n, W, hop, tau_min, tau_max, sample_rate, L)


def frame_candidates(dp, tau_min, tau_max, sample_rate, ft):
    """One frame: the kept candidates as rows (f0, ap, logf) by ascending lag, and their lags."""
    lags = [tau for tau in range(max(tau_min, 2), tau_max + 1)
            if dp[tau] < dp[tau - 1] and (tau == tau_max or dp[tau] <= dp[tau + 1]) and dp[tau] < 1]
    kept = sorted(sorted(lags, key=lambda tau: (dp[tau], tau))[:MAX_CANDIDATES])
    rows = []
    for tau in kept:
        # f0_ref._pick over the lags [tau, tau_max] at a threshold above every candidate's d' < 1: it takes tau, does not advance
        # (d'(tau + 1) is not below d'(tau)), and refines under the contract's conditions
        f0, ap, ts, _ = R._pick(dp, tau, tau_max, ft(2.0), ft(sample_rate), ft)
        assert ts == tau
        rows.append((f0, ap, ft(np.log2(np.float64(f0)))))
    return rows, kept


def _candidates(rows, T, tau_min, tau_max, sample_rate, ft):
    cf, ca, cl = np.zeros((T, MAX_CANDIDATES), dtype=ft), np.ones((T, MAX_CANDIDATES), dtype=ft), np.zeros((T, MAX_CANDIDATES), dtype=ft)
    count, lags = np.zeros(T, dtype=np.int32), np.zeros((T, MAX_CANDIDATES), dtype=np.int64)
    for t, dp in enumerate(rows[:T]):
        got, kept = frame_candidates(dp, tau_min, tau_max, sample_rate, ft)
        count[t] = len(got)
        for k, (f0, ap, logf) in enumerate(got):
            cf[t, k], ca[t, k], cl[t, k], lags[t, k] = f0, ap, logf, kept[k]
    return cf, ca, cl, count, lags


def candidates_f32(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, sample_rate=22050.0, L=None, lags=False):
    L = len(x) if L is None else L
    out = _candidates(dprime_f32(x, n, W, hop, tau_min, tau_max, sample_rate, L), 1 + L // hop, tau_min, tau_max, sample_rate, np.float32)
    assert all(a.dtype == np.float32 for a in out[:3])
    return out if lags else out[:4]


def candidates_f64(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, sample_rate=22050.0, L=None, lags=False):
    L = len(x) if L is None else L
    out = _candidates(dprime_f64(x, n, W, hop, tau_min, tau_max, sample_rate, L), 1 + L // hop, tau_min, tau_max, sample_rate, np.float64)
    return out if lags else out[:4]


def _viterbi(cand_logf, cand_ap, cand_f0, count, frames, logf_top, octave_cost, jump_cost, vuv_cost, unvoiced_cost, ft):
    logf, cap, cf0 = (np.asarray(a) for a in (cand_logf, cand_ap, cand_f0))
    T = logf.shape[0]
    cnt = np.clip(np.asarray(count).astype(np.int64), 0, MAX_CANDIDATES)
    Tb = T if frames is None else max(0, min(int(frames), T))
    top, oc, jc, vc, uc, zero = ft(logf_top), ft(octave_cost), ft(jump_cost), ft(vuv_cost), ft(unvoiced_cost), ft(0.0)
    state, f0, ap = np.full(T, -1, dtype=np.int32), np.zeros(T, dtype=ft), np.ones(T, dtype=ft)
    if Tb == 0:
        return state, zero, f0, ap
    back = np.zeros((Tb, MAX_CANDIDATES + 1), dtype=np.int64)
    D = None
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(Tb):
            lt = [ft(v) for v in logf[t, :cnt[t]]]              # slots past count are never read
            local = [uc] + [ft(cap[t, k]) + oc * (top - lt[k]) for k in range(cnt[t])]
            if t == 0:
                D = local
            else:
                new = []
                for k in range(cnt[t] + 1):
                    best, arg = None, 0
                    for j in range(cnt[t - 1] + 1):
                        if j == 0:
                            trans = zero if k == 0 else vc
                        else:
                            trans = vc if k == 0 else jc * abs(lt[k - 1] - lprev[j - 1])
                        c = D[j] + trans
                        if j == 0 or c < best:
                            best, arg = c, j
                    back[t, k] = arg
                    new.append(local[k] + best)
                D = new
            assert all(type(v) is ft for v in D)
            lprev = lt
    s, cost = 0, D[0]
    for k in range(1, len(D)):
        if D[k] < cost:
            s, cost = k, D[k]
    for t in range(Tb - 1, -1, -1):
        state[t] = s
        if s > 0:
            f0[t], ap[t] = cf0[t, s - 1], cap[t, s - 1]
        else:
            least = ft(1.0)
            for k in range(cnt[t]):
                if k == 0 or cap[t, k] < least:
                    least = ft(cap[t, k])
            ap[t] = least
        s = int(back[t, s])
    return state, cost, f0, ap


def prototype_signal():
    """The signal the tracker was prototyped on: a 150 -> 220 Hz glide of four harmonics with a weak-fundamental stretch, a noise
    burst, a noise tail and silence -> (x fp32, the true F0 per sample, sr, W, hop, tau_min, tau_max)."""
    sr = 22050
    n = int(1.6 * sr)
    t = np.arange(n) / sr
    f = 150 + 70 * t / t[-1]
    ph = 2 * np.pi * np.cumsum(f) / sr
    a1 = np.where((t > 0.5) & (t < 0.58), 0.15, 1.0)
    x = a1 * np.sin(ph) + 0.9 * np.sin(2 * ph) + 0.4 * a1 * np.sin(3 * ph) + 0.3 * np.sin(4 * ph)
    rs = np.random.RandomState(0)
    burst = (t > 0.9) & (t < 0.95)
    x[burst] += 0.55 * rs.randn(int(burst.sum()))
    tail = t > 1.25
    x[tail] = 0.05 * rs.randn(int(tail.sum()))
    x[t > 1.45] = 0
    x *= 0.3
    return x.astype(np.float32), f, sr, 1024, 256, 45, 339


def prototype_frames(n, sr, W, hop):
    """(voiced, tail): the frames centred before 1.25 s - W / 2 samples, and after 1.25 s + W / 2 samples."""
    centre = np.arange(1 + n // hop) * hop / sr
    return centre < 1.25 - W / 2 / sr, centre > 1.25 + W / 2 / sr


def hand_cases():
    """Hand-built candidate tensors whose costs are small multiples of 0.25, so every sum is exact in fp32 and in fp64:
    name -> (cand_logf (T, 8), cand_ap, cand_f0, count (T,), frames or None, the costs, the states expected (T,), the cost expected).
    cand_f0 = 100 * (slot + 1) + t, so that a gathered f0 names its slot and frame."""
    def build(rows):
        T = len(rows)
        logf, ap = np.zeros((T, MAX_CANDIDATES), dtype=np.float32), np.ones((T, MAX_CANDIDATES), dtype=np.float32)
        f0, count = np.zeros((T, MAX_CANDIDATES), dtype=np.float32), np.zeros(T, dtype=np.int32)
        for t, row in enumerate(rows):
            count[t] = len(row)
            for k, (lf, a) in enumerate(row):
                logf[t, k], ap[t, k], f0[t, k] = lf, a, 100.0 * (k + 1) + t
        return logf, ap, f0, count

    flat = dict(logf_top=0.0, octave_cost=0.0, jump_cost=1.0, vuv_cost=0.25, unvoiced_cost=2.0)
    cases = {}
    # frame 0's two candidates cost 0.25 each and lie 0.5 octaves either side of frame 1's: both ways cost 0.75
    cases["tie_between_predecessors"] = (*build([[(1.0, 0.25), (2.0, 0.25)], [(1.5, 0.0)]]), None, flat, [1, 1], 0.75)
    # the last frame's unvoiced state and both candidates cost 0.5
    cases["tie_at_the_end"] = (*build([[(1.0, 0.5), (1.0, 0.5)]]), None, dict(flat, unvoiced_cost=0.5), [0], 0.5)
    cases["tie_at_the_end_voiced"] = (*build([[(3.0, 1.0), (1.0, 0.5), (1.0, 0.5)]]), None, flat, [2], 0.5)
    cases["one_frame"] = (*build([[(1.0, 0.75), (2.0, 0.25), (3.0, 0.5)]]), None, flat, [2], 0.25)
    # octave_cost at work: local = ap + 0.5 * (4 - logf) = 1.75, 0.75, 1.0
    cases["one_frame_octave_cost"] = (*build([[(1.0, 0.25), (3.0, 0.25), (3.5, 0.75)]]), None, dict(flat, logf_top=4.0, octave_cost=0.5), [2], 0.75)
    # a frame without candidates between voiced frames: 0.25 + (0.25 + 2.0) + (0.25 + 0.5)
    cases["no_candidates_between"] = (*build([[(1.0, 0.25)], [], [(1.0, 0.5)]]), None, flat, [1, 0, 1], 3.25)
    cases["frames_0"] = (*build([[(1.0, 0.25)], [(1.0, 0.25)]]), 0, flat, [-1, -1], 0.0)
    cases["frames_1_of_3"] = (*build([[(1.0, 0.25)], [(1.0, 0.25)], [(1.0, 0.25)]]), 1, flat, [1, -1, -1], 0.25)
    cases["all_unvoiced"] = (*build([[], [], [], []]), None, flat, [0, 0, 0, 0], 8.0)
    # candidates too dear to visit: unvoiced throughout although every frame has some
    cases["all_unvoiced_dear"] = (*build([[(1.0, 2.5)], [(1.0, 2.25), (2.0, 3.0)], [(1.0, 2.5)]]), None, flat, [0, 0, 0], 6.0)
    # vuv_cost = 0: switching is free, each frame takes its cheapest state; frame 1's candidate is a 2-octave jump away
    cases["vuv_cost_0"] = (*build([[(1.0, 0.25)], [(3.0, 0.5)], [(1.0, 0.25)]]), None, dict(flat, vuv_cost=0.0, unvoiced_cost=0.75), [1, 0, 1], 1.25)
    return cases


def viterbi_f32(cand_logf, cand_ap, cand_f0, count, frames=None, logf_top=0.0, octave_cost=0.01, jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3):
    return _viterbi(cand_logf, cand_ap, cand_f0, count, frames, logf_top, octave_cost, jump_cost, vuv_cost, unvoiced_cost, np.float32)


def viterbi_f64(cand_logf, cand_ap, cand_f0, count, frames=None, logf_top=0.0, octave_cost=0.01, jump_cost=0.35, vuv_cost=0.14, unvoiced_cost=0.3):
    return _viterbi(cand_logf, cand_ap, cand_f0, count, frames, logf_top, octave_cost, jump_cost, vuv_cost, unvoiced_cost, np.float64)
