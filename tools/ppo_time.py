"""Time the device PPO update (DevicePPO.train_from_arrays: the upload, the whitening, LL_old,
every Adam step in one-workgroup launches of csrc/amx_bcfit.hip, the two EVAL passes) at
run_amp.py's default shape, against the host path it replaces on the same box: the reference's
PPO.train_from_paths loop (mjrl/mjrl/algos/ppo_clip.py:58-103) restated in fp32 torch on the CPU
(tests/ppo_ref.py, the tests' comparator) with the box's share of threads, and against the
parent kernel's step: amx_bcfit_steps with the MLE loss on the same rows and batches, in the
same run.

The device update is timed with events around the whole call, host arrays in and the results
out, after a warm-up call; every call starts from the same parameters and a fresh Adam state,
and the device and the host use the same index batches.  The steps alone (one amx_ppo_steps /
amx_bcfit_steps launch over all of them, alternating) are timed from device-resident inputs.

usage: python tools/ppo_time.py [out.txt] [N] [cpu_threads]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import amp_extensions_amd as amx  # noqa: E402
import ppo_ref as R  # noqa: E402
from amp_extensions_amd import _native as N_  # noqa: E402
from amp_extensions_amd.npg import pack_policy, unpack_policy  # noqa: E402
from amp_extensions_amd.policy import init_mlp_policy_params  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "ppo_time.txt")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10240
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
S, A, EPOCHS, LR, CLIP = 197, 36, 10, 3e-4, 0.2  # mjrl PPO's defaults, actor (32, 32)
steps = EPOCHS * (N // 64)
REPEATS = 5

flat = pack_policy(*init_mlp_policy_params(S, A, seed=123, init_log_std=-0.25))
obs, act, adv = R.concat(R.make_paths((N,), S, A, flat, seed=5))
np.random.seed(77)
batch_sets = [amx.plan_bc_batches(N, EPOCHS) for _ in range(REPEATS + 1)]

ctx = amx.AmxContext(S, A, n_models=1, hidden=16, n_hidden=1, feat_dim=256, device="cuda")


def device_update(batches):
    d = amx.DevicePPO(ctx, *unpack_policy(flat, S, A), clip_coef=CLIP, epochs=EPOCHS, learn_rate=LR)
    return d, d.train_from_arrays(obs, act, adv, batches=batches)


device_update(batch_sets[0])  # warm-up: code objects, allocator
torch.cuda.synchronize()
call_ms = []
for batches in batch_sets[1:]:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    d, dev_out = device_update(batches)  # returns after its one host sync
    e1.record()
    torch.cuda.synchronize()
    call_ms.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
dev_clipped = int(d.step_clipped.sum())

# the steps alone: one launch over all of them, inputs already on the device; PPO and BC's MLE
# step (the parent's kernel) alternate
obs_d, act_d = (torch.from_numpy(x).float().cuda() for x in (obs, act))
adv_d = dev_out["advantages"].float()
idx_d = torch.from_numpy(batch_sets[-1].reshape(steps, 64)).cuda()
losses = torch.zeros(steps, dtype=torch.float32, device="cuda")
clipped = torch.zeros(steps, dtype=torch.int32, device="cuda")
ll_old = torch.empty(N, dtype=torch.float32, device="cuda")
theta0 = torch.from_numpy(flat).cuda()
N_.check(ctx.lib.amx_ppo_old_ll(ctx.h, N, obs_d.data_ptr(), S, act_d.data_ptr(), A, theta0.data_ptr(),
                                ll_old.data_ptr(), ctx.stream), "amx_ppo_old_ll")


def launch(kind):
    theta = theta0.clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if kind == "ppo":
        N_.check(ctx.lib.amx_ppo_steps(ctx.h, N, obs_d.data_ptr(), S, act_d.data_ptr(), A, adv_d.data_ptr(),
                                       ll_old.data_ptr(), None, N_.AMX_PPO_OLD_SNAPSHOT, idx_d.data_ptr(), steps,
                                       theta.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), LR, 0.9, 0.999,
                                       1e-8, CLIP, losses.data_ptr(), clipped.data_ptr(), ctx.stream), "amx_ppo_steps")
    else:
        N_.check(ctx.lib.amx_bcfit_steps(ctx.h, N, obs_d.data_ptr(), S, act_d.data_ptr(), A, idx_d.data_ptr(), steps,
                                         theta.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), LR, 0.9, 0.999,
                                         1e-8, 0.0, N_.AMX_BC_MLE, losses.data_ptr(), ctx.stream), "amx_bcfit_steps")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), theta


step_ms = {"ppo": [], "bc": []}
for rep in range(REPEATS + 1):
    for kind in ("ppo", "bc"):
        ms, theta = launch(kind)
        if rep:
            step_ms[kind].append(ms)
        if kind == "ppo":
            theta_ppo = theta
assert torch.equal(theta_ppo, d.theta)  # the same update as the last timed call (nothing clamped at -3)

# the host path: the reference loop in fp32 on the CPU
torch.set_num_threads(threads)
R.Host(flat, S, A, torch.float32, lr=LR, clip_coef=CLIP).update(obs, act, adv, batch_sets[0][:1, :50])  # warm-up
host = R.Host(flat, S, A, torch.float32, lr=LR, clip_coef=CLIP)
t0 = time.perf_counter()
host_out = host.update(obs, act, adv, batch_sets[-1])
host_ms = (time.perf_counter() - t0) * 1e3

med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
ev = [e for e, _ in call_ms]
ppo_us, bc_us = (med(step_ms[k]) / steps * 1e3 for k in ("ppo", "bc"))
lines = [
    f"PPO policy update, N={N} rows, S/A={S}/{A}, hidden (32, 32), batch 64, {EPOCHS} epochs = {steps} Adam steps, "
    f"clip {CLIP}, lr {LR}, snapshot mode",
    f"device ({torch.cuda.get_device_name(0)}): DevicePPO.train_from_arrays from host arrays, events around the whole "
    f"call (upload, whitening, surr_before, LL_old, the steps, surr_after / kl_dist, read-back), {len(ev)} calls after "
    "a warm-up: " + ", ".join(f"{e:.2f}" for e in ev) + f" ms (median {med(ev):.2f} ms, min {min(ev):.2f}, max "
    f"{max(ev):.2f}; {med(ev) / steps * 1e3:.2f} us per step; host clock: "
    + ", ".join(f"{h:.2f}" for _, h in call_ms) + " ms)",
    f"device, amx_ppo_steps alone ({steps} steps in one launch of one workgroup, inputs resident), "
    f"{len(step_ms['ppo'])} launches after a warm-up: " + ", ".join(f"{e:.2f}" for e in step_ms["ppo"])
    + f" ms (median {med(step_ms['ppo']):.2f} ms, {ppo_us:.2f} us per step)",
    f"device, amx_bcfit_steps (MLE) alone on the same rows and batches, alternating with the above: "
    + ", ".join(f"{e:.2f}" for e in step_ms["bc"]) + f" ms (median {med(step_ms['bc']):.2f} ms, {bc_us:.2f} us per "
    f"step); PPO step / BC step: x{ppo_us / bc_us:.3f}",
    f"host (torch {torch.__version__} CPU, {threads} threads): the restated train_from_paths loop in fp32, one call: "
    f"{host_ms:.1f} ms ({host_ms / steps * 1e3:.1f} us per step)",
    f"ratio host / device call: x{host_ms / med(ev):.1f}",
    f"same parameters and batches: device surr_after {dev_out['surr_after']:.8f} kl_dist {dev_out['kl_dist']:.8f} "
    f"clipped row uses {dev_clipped}; host surr_after {host_out['surr_after']:.8f} kl_dist {host_out['kl_dist']:.8f} "
    f"clipped row uses {int(host_out['step_clipped'].sum())}; "
    f"max |theta device - host| {float(np.max(np.abs(d.theta.cpu().numpy() - host.flat()))):.3g}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
