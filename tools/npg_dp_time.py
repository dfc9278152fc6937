"""Time the data-parallel NPG update (DeviceNPG.train_from_arrays(..., allreduce=...)) on one GPU at
the rollout shape 40 960 x 197 / 36, and write profiles/npg_dp_time.txt:

  * the plain single-process update (the parent commit's path: allreduce=None);
  * the same update through the message path with an all-reduce that does nothing (the cost of the
    extra launches and of the second host sync alone);
  * the same through a one-rank RCCL group (the "nccl" backend, built as tools/rccl_rehearsal.py
    builds it): cg_iters + 4 small collectives more (cg_iters + 3 without whitening);
  * a rank's share at N = 8: 5 120 rows with n_total = 40 960 (rank 0 of a world of 8 whose other
    seven row counts are filled in by the stand-in all-reduce; their whitening records stay empty),
    against the plain update on the same 5 120 rows.  An initialised group overrides rank / world,
    so this one runs before the group exists, on the all-reduce that does nothing else.

Consecutive updates, each with its host syncs, in alternating rounds in one process.  Multi-GPU
RCCL runs need one GPU per rank and are not measured here.

usage: python tools/npg_dp_time.py [--reps 20] [--rounds 3] [--out profiles/npg_dp_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, A, SHARE, WORLD = 40960, 197, 36, 5120, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npg_dp_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("npg_dp_time: no GPU (this tool measures on the device only)")
    sys.path.insert(0, ROOT)
    import amp_extensions_amd as amx
    from amp_extensions_amd.policy import init_mlp_policy_params
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    layers, ls = init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25)
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=dev)
    rs = np.random.RandomState(0)
    obs = torch.from_numpy((0.5 * rs.randn(N, S)).astype(np.float32)).to(dev)
    act = torch.from_numpy(rs.randn(N, A).astype(np.float32)).to(dev)
    adv = torch.from_numpy(rs.randn(N)).to(dev)

    def nothing(t):
        return t

    def rccl(t):
        dist.all_reduce(t)

    def share(t):  # the other seven ranks' row counts
        if t.dtype == torch.int64:
            t[t == 0] = SHARE

    before = [("plain update, 40 960 rows (allreduce=None)", N, {}),
              ("message path, all-reduce that does nothing", N, dict(allreduce=nothing)),
              ("plain update, 5 120 rows", SHARE, {}),
              ("message path, 5 120 rows of n_total 40 960, all-reduce that does nothing else", SHARE,
               dict(allreduce=share, rank=0, world=WORLD))]
    group = [("plain update, 40 960 rows, with the group up", N, {}),
             ("message path, one-rank RCCL group", N, dict(allreduce=rccl))]
    res = {c[0]: [] for c in before + group}
    for _ in range(args.rounds):
        measure(amx, ctx, layers, ls, obs, act, adv, before, res, args.reps)
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29533")):
        os.environ.setdefault(k, v)
    dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1)
    for _ in range(args.rounds):
        measure(amx, ctx, layers, ls, obs, act, adv, group, res, args.reps)
    dist.destroy_process_group()
    report(res, args)


def measure(amx, ctx, layers, ls, obs, act, adv, configs, res, reps):
    for name, n, kw in configs:
        npg = amx.DeviceNPG(ctx, layers, ls, normalized_step_size=0.1, min_log_std=-2.0)

        def run(npg=npg, n=n, kw=kw):
            return npg.train_from_arrays(obs[:n], act[:n], adv[:n], **kw)
        for _ in range(3):
            out = run()
        assert kw.get("world") is None or out["n_total"] == N
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / reps * 1e3)
        print(f"[npg_dp_time] {name}: {res[name][-1]:.3f} ms", file=sys.stderr, flush=True)


def report(res, args):
    lines = [f"Data-parallel NPG update on one GPU, {S} / {A}, 10 CG iterations, whitening on "
             f"({torch.cuda.get_device_name(0)})",
             f"ms per update (consecutive updates with their host syncs, {args.reps} per figure; {args.rounds} "
             "alternating rounds, every round listed)", ""]
    for name, v in res.items():
        lines.append(f"  {name + ':':<82}" + "  ".join(f"{x:.3f}" for x in v))
    lines += ["", "The message path adds per update: one launch per CG iteration (the [P] message), the count",
              "exchange with its host sync, and cg_iters + 4 collectives.  Multi-GPU RCCL runs (one GPU per",
              "rank) are not measured."]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
