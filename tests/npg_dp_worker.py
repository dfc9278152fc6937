"""Worker process of tests/test_gpu_npg_dp_ranks.py (started fresh by the test; not collected).

usage: python npg_dp_worker.py RANK WORLD PORT OUT.npz

One rank of a data-parallel NPG update on the GPU (the ranks share one card).  The ranks'
exchanges are DeviceNPG's collectives, summed by gloo over host copies (RCCL on the multi-GPU
path), each counted.  The cases run one after another in the same process group, so a rank that
took one collective more or fewer than the other in any case would leave the next case waiting or
wrong:
  refused  a BC term: NotImplementedError before any collective;
  empty    rank 0 holds no rows, rank 1 holds 64: the same ValueError on both, after one collective;
  exact    512 rows each of npg_pass_ref.inputs(197, 36, 1024), whiten=False;
  uneven   200 and 549 rows of npg_pass_ref.inputs(197, 36, 749), whiten=True.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

S, A = 197, 36
SPLITS = {"empty": (64, [0, 0, 64]), "exact": (1024, [0, 512, 1024]), "uneven": (749, [0, 200, 749])}
NPG_ARGS = dict(normalized_step_size=0.05, min_log_std=-2.0, FIM_invert_args={"iters": 10, "damping": 1e-4})


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch.distributed as dist

    import amp_extensions_amd as amx
    import npg_pass_ref as P
    from amp_extensions_amd.npg import unpack_policy
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []

    def allreduce(t):  # gloo reduces host tensors: copy out, reduce, copy back
        calls.append(tuple(t.shape))
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=dev)

    def npg_for(n):
        d = P.inputs(S, A, n)
        layers, ls = unpack_policy(d["theta"], S, A)
        return amx.DeviceNPG(ctx, layers, ls, **NPG_ARGS), d

    res = {}
    # ---- refused: decided from the arguments, before the first collective ----------------------
    npg, d = npg_for(64)
    try:
        npg.train_from_arrays(d["obs"], d["act"], d["adv"], bc=(d["obs"][:8], d["act"][:8], 0.1),
                              allreduce=allreduce)  # rank and world: the process group's
        res["refused_error"] = ""
    except NotImplementedError as e:
        res["refused_error"] = f"NotImplementedError: {e}"
    res["refused_calls"] = len(calls)
    # ---- the three splits ----------------------------------------------------------------------
    for case, (n, edges) in SPLITS.items():
        npg, d = npg_for(n)
        lo, hi = edges[rank], edges[rank + 1]
        del calls[:]
        try:
            o = npg.train_from_arrays(d["obs"][lo:hi], d["act"][lo:hi], d["adv"][lo:hi], whiten=case == "uneven",
                                      allreduce=allreduce)
            torch.cuda.synchronize()
            res.update({f"{case}_theta": npg.theta.cpu().numpy(), f"{case}_vpg": o["vpg_grad"].cpu().numpy(),
                        f"{case}_npg": o["npg_grad"].cpu().numpy(), f"{case}_adv": o["advantages"].cpu().numpy(),
                        f"{case}_scal": np.array([o["alpha"], o["delta"], o["surr_after"], o["kl_dist"]]),
                        f"{case}_n_total": o["n_total"]})
            res[f"{case}_error"] = ""
        except ValueError as e:
            res[f"{case}_error"] = f"ValueError: {e}"
        res[f"{case}_calls"] = np.array([int(np.prod(s)) for s in calls])
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
