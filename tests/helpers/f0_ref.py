"""Host restatements of include/nsg.h's nsg_audio_f0 (YIN) and nsg_f0_path_stats (numpy only; no kernel, no torch).

  * yin_f32(x, ...): the contract operation for operation in fp32, in the header's order -- what the kernel must return bit for
    bit.  d(tau) is one fp32 chain per lag over j ascending (numpy rounds every elementwise operation and fuses nothing); the
    running sum takes the lags in groups of 8 (the chain inside a group, the chain over the earlier groups' totals, one add);
    fp32 division is correctly rounded.
  * yin_f64(x, ...): the same definition in plain fp64, sums in numpy's own order -- the independent check.  With detail=True it
    also returns, per frame, the lag chosen and d' at it and at its two neighbours (NaN where there is none).
  * path_stats_f64(f0_a, f0_b, path, steps): the ten sums of nsg_f0_path_stats for one pair.

Both yin functions take one clip x (1-D) of which the first n samples count (default all), zero outside [0, n), and return
(f0 (T,), ap (T,)) for T = 1 + L // hop frames (L defaults to len(x)); frames past 1 + n // hop are (0, 1)."""
import numpy as np

LAG_GROUP = 8            # include/nsg.h: NSG_F0_LAG_GROUP


def _spans(x, n, W, hop, tau_max, dtype):
    """(T_b, W + tau_max + 1) array: row t holds x[t hop - W/2 + i], i = 0 .. W + tau_max, zero outside [0, n)."""
    Tb = 1 + n // hop
    span = W + tau_max + 1
    buf = np.zeros(W // 2 + max(n, (Tb - 1) * hop + span) + span, dtype=dtype)
    buf[W // 2:W // 2 + n] = np.asarray(x[:n], dtype=dtype)
    return buf[np.arange(Tb)[:, None] * hop + np.arange(span)[None, :]]


def _pick(dp, tau_min, tau_max, threshold, sample_rate, ft):
    """One frame's search and refinement over dp[1 .. tau_max] (dp[0] unused), every operation in the type ft."""
    lags = np.arange(tau_min, tau_max + 1)
    below = np.flatnonzero(dp[tau_min:tau_max + 1] < threshold)
    if len(below) == 0:
        return ft(0.0), dp[tau_min:tau_max + 1].min(), 0, (np.nan, np.nan, np.nan)
    ts = int(lags[below[0]])
    while ts + 1 <= tau_max and dp[ts + 1] < dp[ts]:
        ts += 1
    b = dp[ts]
    delta = ft(0.0)
    a = c = ft(np.nan)
    if ts - 1 >= 1 and ts + 1 <= tau_max:
        a, c = dp[ts - 1], dp[ts + 1]
        den = (a - ft(2.0) * b) + c
        if a >= b and c >= b and den > 0:
            delta = (ft(0.5) * (a - c)) / den
    period = ft(ts) + delta
    return ft(sample_rate) / period, b, ts, (a, b, c)


def yin_f32(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, threshold=0.1, sample_rate=22050.0, L=None):
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    L = len(x) if L is None else L
    n = len(x) if n is None else max(0, min(int(n), L))
    T, Tb = 1 + L // hop, 1 + n // hop
    fr = _spans(x, n, W, hop, tau_max, f32)
    d = np.zeros((Tb, tau_max + 1), dtype=f32)                    # column tau; column 0 is the lag 0 nobody reads
    for j in range(W):                                            # one chain per lag, j ascending
        t = fr[:, j:j + 1] - fr[:, j:j + tau_max + 1]
        d = d + t * t
    assert d.dtype == f32
    ng = -(-tau_max // LAG_GROUP)
    dg = np.zeros((Tb, ng * LAG_GROUP), dtype=f32)
    dg[:, :tau_max] = d[:, 1:]
    dg = dg.reshape(Tb, ng, LAG_GROUP)
    p = np.empty_like(dg)                                         # the chain inside a group
    p[:, :, 0] = dg[:, :, 0]
    for r in range(1, LAG_GROUP):
        p[:, :, r] = p[:, :, r - 1] + dg[:, :, r]
    G = np.zeros((Tb, ng), dtype=f32)                             # the chain over the earlier groups' totals, from +0.0
    for g in range(1, ng):
        G[:, g] = G[:, g - 1] + p[:, g - 1, LAG_GROUP - 1]
    c = (G[:, :, None] + p).reshape(Tb, ng * LAG_GROUP)[:, :tau_max]
    num = d[:, 1:] * np.arange(1, tau_max + 1, dtype=f32)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = np.where(c > 0, num / c, f32(1.0)).astype(f32)
    assert c.dtype == f32 and num.dtype == f32
    dp = np.concatenate((np.zeros((Tb, 1), dtype=f32), dp), axis=1)
    f0, ap = np.zeros(T, dtype=f32), np.ones(T, dtype=f32)
    for t in range(min(T, Tb)):
        f0[t], ap[t], _, _ = _pick(dp[t], tau_min, tau_max, f32(threshold), f32(sample_rate), f32)
    return f0, ap


def yin_f64(x, n=None, W=1024, hop=256, tau_min=45, tau_max=339, threshold=0.1, sample_rate=22050.0, L=None, detail=False):
    x = np.asarray(x, dtype=np.float64)
    L = len(x) if L is None else L
    n = len(x) if n is None else max(0, min(int(n), L))
    T, Tb = 1 + L // hop, 1 + n // hop
    fr = _spans(x, n, W, hop, tau_max, np.float64)
    d = np.zeros((Tb, tau_max + 1))
    for tau in range(1, tau_max + 1):
        d[:, tau] = ((fr[:, :W] - fr[:, tau:tau + W]) ** 2).sum(axis=1)
    c = np.cumsum(d[:, 1:], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = np.where(c > 0, d[:, 1:] * np.arange(1, tau_max + 1)[None, :] / c, 1.0)
    dp = np.concatenate((np.zeros((Tb, 1)), dp), axis=1)
    f0, ap = np.zeros(T), np.ones(T)
    lag, abc = np.zeros(T, dtype=np.int64), np.full((T, 3), np.nan)
    for t in range(min(T, Tb)):
        f0[t], ap[t], lag[t], abc[t] = _pick(dp[t], tau_min, tau_max, float(threshold), float(sample_rate), np.float64)
    return (f0, ap, lag, abc) if detail else (f0, ap)


def path_stats_f64(f0_a, f0_b, path, steps):
    """{steps, n_vv, n_a_only, n_b_only, sum x, sum y, sum x^2, sum y^2, sum x y, sum (x - y)^2} over path[:steps], x, y = log2 f0 on
    the cells both voice; also returns the sums of the terms' magnitudes (for a bound on the order of summation)."""
    fa, fb = np.asarray(f0_a, dtype=np.float64), np.asarray(f0_b, dtype=np.float64)
    cells = np.asarray(path)[:steps]
    va, vb = fa[cells[:, 0]], fb[cells[:, 1]]
    a_on, b_on = va > 0, vb > 0
    both = a_on & b_on
    x, y = np.log2(va[both]), np.log2(vb[both])
    terms = [x, y, x * x, y * y, x * y, (x - y) ** 2]
    stats = np.array([steps, both.sum(), (a_on & ~b_on).sum(), (b_on & ~a_on).sum()] + [t.sum() for t in terms], dtype=np.float64)
    return stats, np.array([np.abs(t).sum() for t in terms])
