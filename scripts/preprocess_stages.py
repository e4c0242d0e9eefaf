"""The device stages of multi-speaker preprocessing on one batch, for a kernel trace: 64 clips x 10 s at 16 kHz through
audio.resample (-> 22050 Hz), audio.trim_silence and audio.melspectrogram, 20 times after a warm-up.  Meant to run under
`rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/preprocess_stages.py`; the per-kernel averages of that run are
the figures in DESIGN.md section 5b.  There is no fallback: without a GPU this fails."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from neural_sound_generation_amd import audio as Au

if not torch.cuda.is_available():
    raise SystemExit("preprocess_stages: needs a GPU (cuda:0)")
B, L, SR_IN, SR_OUT, CALLS = 64, 160000, 16000, 22050, 20
g = torch.Generator().manual_seed(0)
t = torch.arange(L) / SR_IN
y = 0.3 * torch.sin(2 * torch.pi * 220.0 * t)[None] * (torch.rand(B, 1, generator=g) + 0.2) + 0.05 * torch.randn(B, L, generator=g)
y[:, :8000] *= 1e-3                                                # half a second of near-silence at each end
y[:, -8000:] *= 1e-3
y = y.to("cuda:0")
for call in range(CALLS + 2):
    z, lens = Au.resample(y, SR_IN, SR_OUT)
    bounds = Au.trim_silence(z, 20.0, lengths=lens)
    mel = Au.melspectrogram(z, lengths=lens)
torch.cuda.synchronize()
print(f"preprocess_stages: {B} clips x {L} samples at {SR_IN} Hz -> {tuple(z.shape)} at {SR_OUT} Hz, bounds[0] = {bounds[0].tolist()}, "
      f"mel {tuple(mel.shape)}; {CALLS + 2} calls of each stage")
