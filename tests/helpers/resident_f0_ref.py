"""Host restatement of include/nsg.h's nsg_collate_f0_bins (numpy only): a gather by the plan, then f0_cond_ref.bins_f32.

  * gather(f0_corpus, plan, T): the rows the definition names -- f_b[t] = f0_corpus[start_b + t] for t < count_b, +0.0 up to T --
    with the kernel's clamps (count into [0, T]; a frame outside [0, corpus_frames) reads as +0.0), so a plan that breaks the
    precondition has a defined answer too.  -> (rows (B, T) fp32, counts (B,) int64 after the clamp).
  * collate_bins_f32(...): bins_f32 of those rows with frames = count -> (bins (B, W) int64, logf (B, W) fp32, rows (B, T) fp32).
  * interior(count, hop, tau_max, frame_length): the crop frames t whose YIN window lies inside the crop on both sides, i.e. the
    frames on which a crop of the whole clip's track and a track of the cropped (zero-padded) audio must agree."""
import numpy as np

from tests.helpers import f0_cond_ref


def gather(f0_corpus, plan, T):
    f0_corpus = np.asarray(f0_corpus, dtype=np.float32)
    plan = np.asarray(plan, dtype=np.int64)
    n = len(f0_corpus)
    start, count = plan[:, 1], np.clip(plan[:, 2], 0, T)
    rows = np.zeros((len(plan), T), dtype=np.float32)
    for b in range(len(plan)):
        for t in range(int(count[b])):
            f = int(start[b]) + t
            if 0 <= f < n:
                rows[b, t] = f0_corpus[f]
    return rows, count


def collate_bins_f32(f0_corpus, plan, T, n_bins, fmin, fmax, W=None, affine=None):
    W = T // 4 if W is None else W
    rows, count = gather(f0_corpus, plan, T)
    bins, logf = f0_cond_ref.bins_f32(rows, W, n_bins, fmin, fmax, frames=count, affine=affine)
    return bins, logf, rows


def interior(count, hop=256, tau_max=339, frame_length=1024):
    """(count,) bool: frame t reads samples t hop - frame_length / 2 .. t hop + frame_length / 2 - 1 + tau_max; interior where
    all of them lie in [0, count hop)."""
    t = np.arange(int(count))
    return (t * hop - frame_length // 2 >= 0) & (t * hop + frame_length // 2 - 1 + tau_max <= int(count) * hop - 1)
