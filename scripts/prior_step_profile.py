"""N steps of PriorTrainStep (GatedPixelCNN(512, 64, 15, 10), B x 20 x 256 codes, full lengths) for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/prior_step_profile.py [--steps 20] [--batch 64]
(no counters, no other tracing; the per-kernel table of the run is quoted in DESIGN.md section 5b)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from neural_sound_generation_amd.prior_train import PriorTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
dev = "cuda:0"
torch.manual_seed(1)
B = args.batch
step = PriorTrainStep(GatedPixelCNN(512, 64, 15, 10).to(dev), lr=3e-4)
x = torch.randint(0, 512, (B, 20, 256), device=dev)
y = torch.randint(0, 10, (B,), device=dev)
full = torch.full((B,), 256, dtype=torch.int64, device=dev)
for _ in range(args.steps):
    loss = step.step(x, y, full, check=False)
torch.cuda.synchronize()
print(f"{args.steps} steps at B={B}: last loss {loss.item():.4f}")
