"""numpy restatement of the codebook usage / revival contract (include/nsg.h: nsg_code_usage, nsg_vq_revive), written from the
rule, not from the kernels: plain Python loops over the codes, Python integers for the row arithmetic."""
import numpy as np


def code_usage_ref(idx, K):
    """-> (counts int64 (K,), perplexity float (fp64), codes in use)."""
    idx = np.asarray(idx).reshape(-1)
    ok = idx[(idx >= 0) & (idx < K)]
    counts = np.bincount(ok, minlength=K).astype(np.int64)
    total = counts.sum()
    if total == 0:
        return counts, 0.0, 0
    p = counts[counts > 0].astype(np.float64) / np.float64(total)
    return counts, float(np.exp(-(p * np.log(p)).sum())), int((counts > 0).sum())


def revive_ref(z, codebook, window, min_count, base_row, stride, adam_m=None, adam_v=None, ema_count=None, ema_sum=None, revive_all=False):
    """z (N, D) fp32 rows.  Returns a dict of the arrays after the revival (copies; None stays None), `slot`, `window`, `revived`
    and `rows` (the row of z each dead code took, in code order)."""
    z = np.asarray(z)
    N = z.shape[0]
    out = {k: (None if a is None else np.array(a, copy=True)) for k, a in
           dict(codebook=codebook, adam_m=adam_m, adam_v=adam_v, ema_count=ema_count, ema_sum=ema_sum).items()}
    K = out["codebook"].shape[0]
    slot = np.full(K, -1, dtype=np.int32)
    rows = []
    j = 0
    for k in range(K):
        if revive_all or int(window[k]) < int(min_count):
            row = (int(base_row) + j * int(stride)) % N
            slot[k] = j
            rows.append(row)
            out["codebook"][k] = z[row]
            if out["adam_m"] is not None:
                out["adam_m"][k] = 0
            if out["adam_v"] is not None:
                out["adam_v"][k] = 0
            if out["ema_count"] is not None:
                out["ema_count"][k] = 1
            if out["ema_sum"] is not None:
                out["ema_sum"][k] = z[row]
            j += 1
    out.update(slot=slot, window=np.zeros(K, dtype=np.int32), revived=j, rows=rows)
    return out
