"""Time the device behaviour-cloning warm start (DeviceBC.fit: the upload, loss_before, every
Adam step in one-workgroup launches of csrc/amx_bcfit.hip, loss_after) at run.py's default
shape, against the host path it replaces on the same box: the reference's BC.fit loop
(mjrl/mjrl/algos/behavior_cloning.py:106-139) restated in fp32 torch on the CPU
(tests/bcfit_ref.py, the tests' comparator) with the box's share of threads.

The device fit is timed with events around the whole call, host arrays in and the three
return values out, after a warm-up fit; every fit starts from the same parameters and a fresh
Adam state, and the device and the host use the same index batches.  The steps alone (one
amx_bcfit_steps launch over all of them) are timed separately from device-resident inputs.

usage: python tools/bcfit_time.py [out.txt] [N] [cpu_threads]
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
import bcfit_ref as B  # noqa: E402
from amp_extensions_amd import _native as N_  # noqa: E402
from amp_extensions_amd.npg import pack_policy  # noqa: E402
from amp_extensions_amd.policy import init_mlp_policy_params  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "bcfit_time.txt")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
S, A, EPOCHS, LR = 197, 36, 3, 1e-3  # run.py: bc_epochs 3, batch 64, lr 1e-3, actor (32, 32)
VFIT_US = 41.1                       # profiles/vfit_time.txt: the value fit's four-launch step
steps = EPOCHS * (N // 64)
REPEATS = 5

obs, act = B.concat(B.make_paths((N,), S, A, seed=5))
flat = pack_policy(*init_mlp_policy_params(S, A, seed=123, init_log_std=-0.25))
np.random.seed(77)
batch_sets = [amx.plan_bc_batches(N, EPOCHS) for _ in range(REPEATS + 1)]

ctx = amx.AmxContext(S, A, n_models=1, hidden=16, n_hidden=1, feat_dim=256, device="cuda")


def device_fit(batches):
    dbc = amx.DeviceBC(ctx, flat, lr=LR, loss_type="MSE")
    return dbc, dbc.fit(obs, act, EPOCHS, batches=batches)


device_fit(batch_sets[0])  # warm-up: code objects, allocator
torch.cuda.synchronize()
fit_ms = []
for batches in batch_sets[1:]:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    dbc, dev_out = device_fit(batches)  # returns after its one host sync
    e1.record()
    torch.cuda.synchronize()
    fit_ms.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))

# the steps alone: one launch over all of them, inputs already on the device
obs_d, act_d = (torch.from_numpy(x).float().cuda() for x in (obs, act))
idx_d = torch.from_numpy(batch_sets[-1].reshape(steps, 64)).cuda()
losses = torch.zeros(steps, dtype=torch.float32, device="cuda")
step_ms = []
for _ in range(REPEATS + 1):
    theta = torch.from_numpy(flat).cuda()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    N_.check(ctx.lib.amx_bcfit_steps(ctx.h, N, obs_d.data_ptr(), S, act_d.data_ptr(), A, idx_d.data_ptr(), steps,
                                     theta.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), LR, 0.9, 0.999, 1e-8,
                                     0.0, N_.AMX_BC_MSE, losses.data_ptr(), ctx.stream), "amx_bcfit_steps")
    e1.record()
    torch.cuda.synchronize()
    step_ms.append(e0.elapsed_time(e1))
step_ms = step_ms[1:]
assert torch.equal(theta, dbc.theta)  # the same fit as the last timed DeviceBC.fit

# the host path: the reference loop in fp32 on the CPU
torch.set_num_threads(threads)
B.Host(flat, S, A, torch.float32, "MSE", lr=LR).fit(obs, act, batch_sets[0][:1, :50])  # warm-up
host = B.Host(flat, S, A, torch.float32, "MSE", lr=LR)
t0 = time.perf_counter()
host_out = host.fit(obs, act, batch_sets[-1])
host_ms = (time.perf_counter() - t0) * 1e3

med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
ev = [e for e, _ in fit_ms]
lines = [
    f"behaviour-cloning warm start, N={N} rows, S/A={S}/{A}, hidden (32, 32), batch 64, {EPOCHS} epochs = {steps} "
    "Adam steps, MSE",
    f"device ({torch.cuda.get_device_name(0)}): DeviceBC.fit from host arrays, events around the whole call (upload, "
    f"loss_before, the steps, loss_after, read-back), {len(ev)} fits after a warm-up: "
    + ", ".join(f"{e:.2f}" for e in ev) + f" ms (median {med(ev):.2f} ms, min {min(ev):.2f}, max {max(ev):.2f}; "
    f"{med(ev) / steps * 1e3:.2f} us per step; host clock: " + ", ".join(f"{h:.2f}" for _, h in fit_ms) + " ms)",
    f"device, amx_bcfit_steps alone ({steps} steps in one launch of one workgroup, inputs resident), {len(step_ms)} "
    "launches after a warm-up: " + ", ".join(f"{e:.2f}" for e in step_ms) + f" ms (median {med(step_ms):.2f} ms, "
    f"{med(step_ms) / steps * 1e3:.2f} us per step; the value fit's four-launch step: {VFIT_US} us, "
    f"x{VFIT_US / (med(step_ms) / steps * 1e3):.2f})",
    f"host (torch {torch.__version__} CPU, {threads} threads): the restated BC.fit loop in fp32, one fit: "
    f"{host_ms:.1f} ms ({host_ms / steps * 1e3:.1f} us per step)",
    f"ratio host / device fit: x{host_ms / med(ev):.1f}",
    f"same parameters and batches: device loss_before {dev_out[0]:.8f} epoch totals "
    f"{[round(x, 6) for x in dev_out[1]]} loss_after {dev_out[2]:.8f}; host loss_before {host_out[0]:.8f} "
    f"epoch totals {[round(x, 6) for x in host_out[1]]} loss_after {host_out[2]:.8f}; "
    f"max |theta device - host| {float(np.max(np.abs(dbc.theta.cpu().numpy() - host.flat()))):.3g}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
