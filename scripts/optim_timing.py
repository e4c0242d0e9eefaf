"""HIP-event times of the optimiser's launches at the bucket sizes of configs[1] (1.25 M floats) and configs[3] (6.8 M floats):
the plain adam_step, grad_sumsq, and adamw_step with every option on (a segment table of 90 tensors, clipping, the guard, the
shadow).  Median of 20 timed calls after 5 warm-up calls; one JSON line per size.  DESIGN.md quotes a single run of this."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_sound_generation_amd import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


for n in (1_250_048, 6_800_000):
    p, g, m, v, shadow = (torch.randn(n, device=DEV) * 1e-2 for _ in range(5))
    v.abs_()
    S = 90
    ends = torch.linspace(n / S, n, S).long() // 64 * 64
    ends[-1] = n
    seg_end, seg_wd = ends.to(DEV), torch.full((S,), 0.01, device=DEV)
    sumsq, stats = torch.zeros(1, dtype=torch.float64, device=DEV), ops.new_adamw_stats(DEV)
    t_adam = timed(lambda: ops.adam_step(p, g, m, v, 7))
    t_sumsq = timed(lambda: ops.grad_sumsq(g, out=sumsq))
    t_adamw = timed(lambda: ops.adamw_step(p, g, m, v, 7, seg_end=seg_end, seg_wd=seg_wd, sumsq=sumsq, max_norm=1.0, skip_nonfinite=True,
                                           shadow=shadow, one_minus_decay=1e-4, stats=stats))
    t_neutral = timed(lambda: ops.adamw_step(p, g, m, v, 7))
    print(json.dumps({"floats": n, "adam_step_us": round(t_adam, 1), "grad_sumsq_us": round(t_sumsq, 1),
                      "adamw_step_all_options_us": round(t_adamw, 1), "adamw_step_neutral_us": round(t_neutral, 1),
                      "adam_step_TBps": round(28.0 * n / t_adam / 1e6, 2), "adamw_step_TBps": round(36.0 * n / t_adamw / 1e6, 2)}))
