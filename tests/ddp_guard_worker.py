"""Worker of tests/test_fused_adam_guard_gpu.py::test_two_ranks_skip_the_same_step: one of TWO processes that share cuda:0
over gloo (see tests/ddp_worker.py for why gloo).  Three steps of the real PlankModel + GradSync + FusedAdam(skip_nonfinite);
on step 2 rank 1 alone poisons its gradient buffer BEFORE the first slice is exchanged, so the all-reduced sum is NaN on both
ranks and both guards must skip that step - with no collective of their own."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch
import torch.distributed as dist

from ddp_worker import build, half


def main(rank, world, port, out_path):
    import large_cases as LC
    from plankassembly_amd.distributed import GradSync
    from plankassembly_amd.optim import FusedAdam
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = LC.CASES["live"]
        m = build(c, "f32")
        sync = GradSync(m, grad_dtype="f32")
        sync.broadcast_parameters(0)
        opt = FusedAdam(m, lr=1e-3, grad_scale=1.0 / world, skip_nonfinite=True)
        mine = m.prepare_batch(half(LC.case_batch(c, batch_size=4), rank, world))
        poison = {"now": False}

        def hook(seg, lo, hi):                       # GradSync's own hook, after this rank's slice was (maybe) poisoned
            if poison["now"] and seg == 0:
                m.grad_sync_buffer[lo] = float("nan")
            sync._on_segment(seg, lo, hi)

        m.register_grad_ready_hook(hook)
        for step in (1, 2, 3):
            poison["now"] = step == 2 and rank == 1
            opt.zero_grad()
            m(mine)["loss"].backward()
            sync.wait()
            opt.step()
        torch.cuda.synchronize()
        stats = opt.guard_stats()
        torch.save({"stats": stats, "params": m.flat_params.detach().cpu().clone(),
                    "finite": bool(torch.isfinite(m.flat_params).all())}, f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]), int(a[1]), int(a[2]), a[3])
