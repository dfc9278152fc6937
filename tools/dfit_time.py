"""Time the device discriminator training (GAILCost.update_disc: amx_dfit_step, csrc/amx_dfit.hip)
and compute_chi2_distance at run_amp's shape -- D = 394 (S = 197), hidden [1024, 512], 256-row
batches sampled from a replay ring of 100 000 rows, 50 000 expert rows, SGD(1e-5, 0.9), least
squares -- against the same two restated in fp32 torch (tests/dfit_ref.py, the tests' comparator)
on the same box's CPU threads.

The device steps are timed with events around all of them after warm-up steps, each step whole
(index draw and upload, the launches, the refresh of the inference copies, the metrics
read-back); both sides start from the same weights and take the same batches, and their last
step's losses are printed side by side.

usage: python tools/dfit_time.py [out.txt] [cpu_threads] [--no-host] [--steps K]
(--no-host: the device part only, for a kernel-trace run of its own)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amp_extensions_amd.costs import GAILCost  # noqa: E402
from amp_extensions_amd.datasets import AgentReplayBuffer  # noqa: E402
import dfit_ref as R  # noqa: E402

argv = sys.argv[1:]
steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 200
args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--steps")]
no_host = "--no-host" in argv
out_path = args[0] if args else os.path.join("profiles", "dfit_time.txt")
threads = int(args[1]) if len(args) > 1 else 16
S, HIDDEN, BS, N_RB, N_EXPERT, WARM, CHI2_REPS, HOST_STEPS = 197, [1024, 512], 256, 100000, 50000, 10, 3, 20
OPT = {"lr": 0.00001, "momentum": 0.9}

expert = R.synthetic_rows(N_EXPERT, S, 1, 0.5, 0.3)
agent = R.synthetic_rows(N_RB, S, 2, 0.7, -0.2)
rb = AgentReplayBuffer(device="cuda", max_size=N_RB)
rb.add(agent[:, :S].cuda(), agent[:, S:].cuda())
gc = GAILCost(expert, agent_rb=rb, hidden_dims=HIDDEN, seed=100, disc_opt="sgd", disc_opt_args=OPT, device="cuda")
init = [w.clone() for pair in gc.weights for w in pair]

np.random.seed(0)
for _ in range(WARM):   # code objects, workspaces
    gc.update_disc(None)
gc.compute_chi2_distance()
np.random.seed(1)
rng = np.random.get_state()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(steps):
    met = gc.update_disc(None)
e1.record()
torch.cuda.synchronize()
step_us = e0.elapsed_time(e1) / steps * 1e3
np.random.seed(2)
t0 = time.perf_counter()
for _ in range(CHI2_REPS):
    chi2 = gc.compute_chi2_distance()   # ends in its read-back
chi2_ms = (time.perf_counter() - t0) / CHI2_REPS * 1e3
lines = [
    f"discriminator training, D {2 * S}, hidden {HIDDEN}, batch {BS} from a ring of {N_RB} rows, {N_EXPERT} expert "
    f"rows, SGD {OPT}, least squares",
    f"device ({torch.cuda.get_device_name(0)}): update_disc, events around {steps} whole steps after {WARM} warm-up "
    f"steps: {step_us:.1f} us per step; compute_chi2_distance ({N_EXPERT} + {N_EXPERT} rows), host clock around "
    f"{CHI2_REPS} calls: {chi2_ms:.2f} ms per call",
]
if not no_host:
    torch.set_num_threads(threads)
    n = min(steps, HOST_STEPS)
    np.random.set_state(rng)
    batches = []
    for _ in range(n):   # the draws of the device's first n timed steps
        idx_m, idx_e = np.random.randint(0, N_RB, BS), np.random.randint(0, N_EXPERT, BS)
        batches.append((expert[idx_e], agent[idx_m]))
    cfg = ("least_squares", "sgd", OPT["lr"], OPT["momentum"], 0.5, 0.05, 10.0, torch.float32)
    R.restate(init, batches[:2], *cfg)   # warm-up
    t0 = time.perf_counter()
    host = R.restate(init, batches, *cfg)
    host_us = (time.perf_counter() - t0) / n * 1e6
    np.random.seed(2)
    a_idx = np.random.randint(0, N_RB, size=N_EXPERT)
    R.chi2(host["weights"], expert[:1000], agent[:1000], 0.5, torch.float32)
    t0 = time.perf_counter()
    for _ in range(CHI2_REPS):
        R.chi2(host["weights"], expert, agent[a_idx], 0.5, torch.float32)
    host_chi2_ms = (time.perf_counter() - t0) / CHI2_REPS * 1e3
    # the device run again for n steps from the same weights and draws, for the loss comparison
    gc.load_weights(gc.weights)
    np.random.set_state(rng)
    for _ in range(n):
        met = gc.update_disc(None)
    lines += [
        f"host (torch {torch.__version__} CPU, {threads} threads, fp32): the restated step (closed-form gradient), "
        f"{n} steps: {host_us:.0f} us per step; the restated chi^2: {host_chi2_ms:.1f} ms per call",
        f"ratio host / device: update_disc x{host_us / step_us:.1f}, "
        f"compute_chi2_distance x{host_chi2_ms / chi2_ms:.1f}",
        f"total_disc_loss of step {n}, same weights and batches: device {met['total_disc_loss']:.6f} host "
        f"{host['metrics'][-1]['total_disc_loss']:.6f}",
    ]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
