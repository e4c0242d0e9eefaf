"""Host restatement of include/nsg.h's nsg_collate_audio (numpy only): a loop over the plan's rows -- slice, zero-pad.

  * collate_audio(corpus, plan, T, hop): out[b][i] = corpus[start_b hop + i] for i < count_b hop, +0.0 up to T hop, with the
    kernel's clamps (count into [0, T]; a sample outside [0, len(corpus)) reads as +0.0), so a plan that breaks the precondition
    has a defined answer too.  -> (B, T hop) fp32; the samples are moved, never computed with, so their bits are the corpus'."""
import numpy as np


def collate_audio(corpus, plan, T, hop):
    corpus = np.asarray(corpus, dtype=np.float32)
    plan = np.asarray(plan, dtype=np.int64)
    n = len(corpus)
    out = np.zeros((len(plan), T * hop), dtype=np.float32)
    for b, (_, start, count) in enumerate(plan.tolist()):
        count = min(max(count, 0), T)
        lo, hi = start * hop, (start + count) * hop                  # (Python integers: no overflow, whatever the plan holds)
        a, z = min(max(lo, 0), n), min(max(hi, 0), n)                # the part of [lo, hi) that is inside the corpus
        if z > a:
            out[b, a - lo:z - lo] = corpus[a:z]
    return out
