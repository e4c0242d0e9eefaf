"""One rank of the two-rank revival rehearsal (tests/test_gpu_codebook_revival.py).  Started as a fresh child process by
tests.helpers.spawn.run_ranks; both ranks share GPU 0 and talk over gloo (NSG_DIST_BACKEND=gloo NSG_DEVICE_INDEX=0), so
FusedTrainStep.step() with revive_every=2 runs its world > 1 branch as it would under torchrun + RCCL: the window's all-reduce,
the kernel on every rank, the codebook's broadcast from rank 0.  Each rank trains on its own batches, in gradient mode and with
the EMA codebook, and writes what it saw and what it holds after the revival step.

    python tests/helpers/revive_rank.py <out dir>        (RANK / WORLD_SIZE / MASTER_* in the env)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    out_dir = sys.argv[1]
    from neural_sound_generation_amd import distributed as D, models as M, ops
    from neural_sound_generation_amd.data import synthetic_mel_batch
    from neural_sound_generation_amd.train import FusedTrainStep

    rank, world, _ = D.init_from_env()
    dev = torch.device("cuda", int(os.environ.get("NSG_DEVICE_INDEX", "0")))
    torch.cuda.set_device(dev)
    out = {}
    real_revive, real_allreduce = ops.vq_revive, D.allreduce_sum_

    for tag, ema in (("grad", None), ("ema", 0.99)):
        seen = {}

        def allreduce(flat, group=None, async_op=False):
            if flat.dtype == torch.int32:                        # the window, before it is summed over the ranks
                seen["local_window"] = flat.cpu().numpy().copy()
            return real_allreduce(flat, group, async_op)

        def revive(rows, codebook, window, **kw):
            seen.update(window=window.cpu().numpy().copy(), codebook_before=codebook.cpu().numpy().copy(), base_row=kw["base_row"],
                        stride=kw["stride"], z=rows.cpu().numpy().copy())
            return real_revive(rows, codebook, window, **kw)

        D.allreduce_sum_, ops.vq_revive = allreduce, revive
        torch.manual_seed(100 + rank)                            # rank 1 starts elsewhere: the step replicates rank 0's state itself
        model = M.VQVAE(1, 16, 32, ema_decay=ema).to(dev).train()
        step = FusedTrainStep(model, lr=1e-3, revive_every=2, revive_min_count=2, revive_seed=9)
        assert step.world == world == 2
        gen = torch.Generator(device=dev).manual_seed(500 + rank)        # every rank its own shard
        for s in (1, 2):
            step.step(synthetic_mel_batch(4, 64, gen, dev))
            out[f"{tag}.idx{s}"] = step.last_indices.cpu().numpy().copy()
        torch.cuda.synchronize()
        D.allreduce_sum_, ops.vq_revive = real_allreduce, real_revive
        w = model.codebook.embedding.weight
        for k, v in seen.items():
            out[f"{tag}.{k}"] = np.asarray(v)
        out[f"{tag}.codebook"] = w.detach().cpu().numpy()
        out[f"{tag}.slot"] = step.reviver.slot.cpu().numpy()
        out[f"{tag}.exp_avg"] = step.opt.exp_avg.cpu().numpy()
        out[f"{tag}.exp_avg_sq"] = step.opt.exp_avg_sq.cpu().numpy()
        if ema is None:
            for p, off in zip(step.opt._params, step.opt.offsets):
                if p is w:
                    out["grad.exp_avg_cb"] = step.opt.exp_avg[off:off + w.numel()].view_as(w).cpu().numpy()
                    out["grad.exp_avg_sq_cb"] = step.opt.exp_avg_sq[off:off + w.numel()].view_as(w).cpu().numpy()
        else:
            out["ema.ema_count"] = model.codebook.ema_count.cpu().numpy()
            out["ema.ema_sum"] = model.codebook.ema_sum.cpu().numpy()
        assert step.codebook_stats()["events"] == 1

    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
