"""Timing of classifier-free guidance in the latent prior's sampler at production width, GatedPixelCNN(512, 64, 15), on
20 x 256 codes with temperature 0.8, top_k 64, top_p 0.95:

  * guided:  32 pairs through nsg_prior_walk_cfg (64 clips in the row pass and in the walk, 32 picks per position);
  * ctl:     64 clips through nsg_prior_walk_ctl, the baseline the guided walk should sit at (the same products, 64 picks);
  * plain:   64 clips through nsg_prior_walk.

Each variant is warmed up once, then the variants are run in turn `--repeats` times; a run reports the GPU milliseconds of
its 20 row passes and of its 20 walks (device events around each phase, GatedPixelCNN._walk_rows(times=)).  Per variant and
phase: the median, the minimum and the maximum over the repeats; `spread` is (max - min) / median.  Prints one JSON line per
variant and appends the run's record, tagged --tag, to the JSON list in --out (default profiles/prior_guidance_timing.json).

--baseline leaves the guided variant out and uses nothing the guided sampler added, so the same file runs unchanged on an
earlier commit's tree: that is how "plain and ctl did not move" is measured, both trees in one session, alternating, each
run a process of its own (the committed file holds parent, this commit, parent, this commit, in the order they ran)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--tag", default="this commit")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--width", type=int, default=256)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prior_guidance_timing.json"))
args = ap.parse_args()

dev = "cuda:0"
torch.manual_seed(1)
N_CLASSES, NULL = 10, 9
m = GatedPixelCNN(512, 64, 15, N_CLASSES).to(dev)
P, H, W = args.pairs, 20, args.width
CTL = (0.8, 64, 0.95)
label = torch.randint(0, N_CLASSES - 1, (2 * P,), device=dev)
pairs = torch.stack([label[:P], torch.full_like(label[:P], NULL)], 1).reshape(-1)
u = torch.rand(2 * P, H, W, device=dev)


def run(variant):
    """One sample of the variant, phase by phase: (row_pass_ms, walk_ms) summed over the H rows."""
    times = {}
    with torch.no_grad():
        if variant == "guided":
            m._walk_rows(pairs, 2 * P, H, W, u=u[:P], codes=torch.empty(P, H, W, dtype=torch.int64, device=dev), times=times, ctl=CTL,
                         guidance=2.0)
        else:
            m._walk_rows(label, 2 * P, H, W, u=u, codes=torch.empty(2 * P, H, W, dtype=torch.int64, device=dev), times=times,
                         ctl=CTL if variant == "ctl" else None)
    return times["row_pass_ms"], times["walk_ms"]


variants = ["plain", "ctl"] + ([] if args.baseline else ["guided"])
for v in variants:                                  # every shape and kernel the timed runs use
    run(v)
runs = {v: [] for v in variants}
for _ in range(args.repeats):                       # in turn, so that a drift of the machine falls on all of them alike
    for v in variants:
        runs[v].append(run(v))


def stats(xs):
    med = statistics.median(xs)
    return {"median": round(med, 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round((max(xs) - min(xs)) / med, 4)}


out = {"tree": args.tag, "model": "GatedPixelCNN(512, 64, 15)", "clips": 2 * P, "pairs": P, "H": H, "W": W, "controls": list(CTL), "repeats": args.repeats,
       "device": torch.cuda.get_device_name(0), "variants": {}}
for v in variants:
    rec = {"row_pass_ms": stats([r for r, _ in runs[v]]), "walk_ms": stats([w for _, w in runs[v]])}
    rec["walk_us_per_position"] = round(rec["walk_ms"]["median"] * 1e3 / (H * W), 2)
    out["variants"][v] = rec
    print(json.dumps(dict(what=v, **rec)), flush=True)
if not args.baseline:
    g, c = out["variants"]["guided"], out["variants"]["ctl"]
    out["guided_over_ctl"] = {"walk": round(g["walk_ms"]["median"] / c["walk_ms"]["median"], 4),
                              "row_pass": round(g["row_pass_ms"]["median"] / c["row_pass_ms"]["median"], 4)}
    print(json.dumps({"what": "guided_over_ctl", **out["guided_over_ctl"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
records = []
if os.path.exists(args.out):
    with open(args.out) as f:
        records = json.load(f)
with open(args.out, "w") as f:
    json.dump(records + [out], f, indent=1)
    f.write("\n")
