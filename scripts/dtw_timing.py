"""Timing of the mel-cepstral-distortion path (audio.mel_cepstral_distortion = two nsg_mel_cepstra launches + one nsg_dtw):
64 and 1024 pairs of 512 x 512 and of 900 x 700 frames, 80 bands, 13 coefficients.  Every shape is warmed up, then timed in
windows of whole calls that end in a device synchronise; the figure is the median window.  Beside it: nsg_dtw alone, the fp32
host restatement (tests/helpers/dtw_ref.py) on one pair of each size -- the only baseline there is -- and the share of an
evaluate.test_conversion batch that the two MCD calls take against the encode / decode they follow.
There is no fallback: without a GPU this fails.    python scripts/dtw_timing.py [--json out.json]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_sound_generation_amd import audio as Au, evaluate, models, ops
from tests.helpers import dtw_ref as R

if not torch.cuda.is_available():
    raise SystemExit("dtw_timing: needs a GPU (cuda:0)")
dev = torch.device("cuda:0")
WINDOWS, MIN_WINDOW_S = 7, 0.25


def median_time(fn):
    """Seconds per call: warm up, size a window to at least MIN_WINDOW_S, take the median of WINDOWS windows."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    times = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) / reps)
    return statistics.median(times), min(times), max(times), reps


results = []
gen = torch.Generator(dev).manual_seed(0)
for la, lb in ((512, 512), (900, 700)):
    ha, hb = np.random.RandomState(1).random_sample((80, la)).astype(np.float32), np.random.RandomState(2).random_sample((80, lb)).astype(np.float32)
    table = Au.cepstra_table(80, 13)
    ca, cb = R.cepstra32(ha, table), R.cepstra32(hb, table)
    t = time.perf_counter()
    host_cost, host_steps, _ = R.dtw32(ca, cb)
    host_s = time.perf_counter() - t
    for B in (64, 1024):
        mel_a, mel_b = torch.rand(B, 80, la, device=dev, generator=gen), torch.rand(B, 80, lb, device=dev, generator=gen)
        mel_a[0].copy_(torch.from_numpy(ha)); mel_b[0].copy_(torch.from_numpy(hb))
        fa, fb = torch.full((B,), la, dtype=torch.int32, device=dev), torch.full((B,), lb, dtype=torch.int32, device=dev)
        mcd, steps = Au.mel_cepstral_distortion(mel_a, mel_b, fa, fb)
        cost0 = float(mcd[0]) * int(steps[0]) / Au.MCD_DB
        assert int(steps[0]) == host_steps and abs(cost0 - float(host_cost)) <= 4e-7 * float(host_cost), (cost0, float(host_cost))
        a, b = Au.mel_cepstra(mel_a, fa), Au.mel_cepstra(mel_b, fb)
        full = median_time(lambda: Au.mel_cepstral_distortion(mel_a, mel_b, fa, fb))
        alone = median_time(lambda: ops.dtw(a, b, fa, fb))
        cells = B * la * lb
        rec = dict(pairs=B, len_a=la, len_b=lb, n_ceps=13, mcd_ms=full[0] * 1e3, mcd_ms_min=full[1] * 1e3, mcd_ms_max=full[2] * 1e3,
                   calls_per_window=full[3], windows=WINDOWS, pairs_per_s=B / full[0], cells_per_s=cells / full[0], dtw_ms=alone[0] * 1e3,
                   dtw_cells_per_s=cells / alone[0], host_restatement_s_per_pair=host_s, host_cells_per_s=la * lb / host_s)
        results.append(rec)
        print(json.dumps(rec), flush=True)

# share of a test_conversion batch: convert_voice (encode + decode) against the two MCD calls that follow it
B, Ts, Tt = 64, 512, 640
model = models.VQVAE(1, 256, 512, n_speakers=4).to(dev).eval()
c_src, c_tgt = torch.rand(B, 80, Ts, device=dev, generator=gen), torch.rand(B, 80, Tt, device=dev, generator=gen)
fs, ft = np.full(B, Ts, dtype=np.int32), np.full(B, Tt, dtype=np.int32)
g = torch.arange(B, dtype=torch.int64) % 4
_, conv = evaluate.convert_voice(model, c_src, g)


def both_mcds():
    Au.mel_cepstral_distortion(conv, c_tgt, fs, ft)
    Au.mel_cepstral_distortion(c_src, c_tgt, fs, ft)


t_conv, t_mcd = median_time(lambda: evaluate.convert_voice(model, c_src, g))[0], median_time(both_mcds)[0]
rec = dict(conversion_batch=dict(clips=B, frames_src=Ts, frames_tgt=Tt, dim=256, codes=512), convert_voice_ms=t_conv * 1e3, two_mcd_ms=t_mcd * 1e3,
           mcd_share=t_mcd / (t_conv + t_mcd))
results.append(rec)
print(json.dumps(rec), flush=True)
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
