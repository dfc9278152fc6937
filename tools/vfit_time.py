"""Time the device value-baseline fit (DeviceMLPBaseline.fit_grid: features + 2 epochs of
batch-64 Adam, csrc/amx_vfit.hip) at bench.py's train shape, against the host path it
replaces on the same box: the reference's fit_data loop (mjrl/mjrl/utils/optimize_model.py:
7-36) in torch on the CPU with the box's share of threads.

The device fit is timed with events around the whole call (feature kernel, permutation draw
and upload, every step's launches), after a warm-up fit; both fits start from the same weights
and use the same permutations, and their epoch losses are printed side by side.

usage: python tools/vfit_time.py [out.txt] [N] [S] [cpu_threads]
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amp_extensions_amd as amx  # noqa: E402
from amp_extensions_amd.gae import init_mlp_baseline_params  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "vfit_time.txt")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40960
S = int(sys.argv[3]) if len(sys.argv) > 3 else 197
threads = int(sys.argv[4]) if len(sys.argv) > 4 else 16
A, L, EPOCHS, LR, REG = 36, 128, 2, 1e-3, 1e-3  # run.py: vf_iters 2, vf_lr 1e-3, vf_reg_coef 1e-3
T = N // L
assert T * L == N
steps = EPOCHS * (N // 64 - 1)

rs = np.random.RandomState(0)
obs = 0.5 * rs.randn(N, S)
ret = rs.randn(N) * 2.0 + 1.0
end = np.zeros(N, dtype=np.uint8)  # engine layout: row t * L + lane, one trajectory per lane
layers = init_mlp_baseline_params(S, (128, 128), seed=7)
perm_sets = [[rs.permutation(N) for _ in range(EPOCHS)] for _ in range(4)]

ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device="cuda")
obs_d, ret_d, end_d = (torch.from_numpy(x).cuda() for x in (obs, ret, end))
bl = amx.DeviceMLPBaseline(ctx, layers, learn_rate=LR, reg_coef=REG, epochs=EPOCHS)


def device_fit(perms, errors=False):
    return bl.fit_grid(N, T, L, obs_d, S, end_d, L, ret_d, perms=perms, return_errors=errors, return_all_errors=errors)


device_fit(perm_sets[0])  # warm-up: code objects, workspaces
torch.cuda.synchronize()
dev_ms = []
for perms in perm_sets[1:]:
    bl.sync_from(layers)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    device_fit(perms)
    e1.record()
    t1 = time.perf_counter()  # every launch enqueued
    torch.cuda.synchronize()
    dev_ms.append((e0.elapsed_time(e1), (t1 - t0) * 1e3))
# the last timed fit again with the reference's return values, for the comparison below
bl = amx.DeviceMLPBaseline(ctx, layers, learn_rate=LR, reg_coef=REG, epochs=EPOCHS)  # fresh Adam state
dev_out = device_fit(perm_sets[-1], errors=True)
torch.cuda.synchronize()

# the host path: MLPBaseline's model, optimizer and fit_data on float32 features
torch.set_num_threads(threads)
feat = np.concatenate([np.clip(obs, -10, 10) / 10.0, np.zeros((N, 4))], axis=1)
tpos = (np.arange(N) // L) / 1000.0
for j in range(4):
    feat[:, S + j] = tpos ** (j + 1)
x, y = torch.from_numpy(feat.astype(np.float32)), torch.from_numpy(ret.astype(np.float32).reshape(-1, 1))


def host_model():
    mods = []
    for i, (W, b) in enumerate(layers):
        lin = nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        mods += [lin] + ([nn.ReLU()] if i < len(layers) - 1 else [])
    model = nn.Sequential(*mods)
    return model, torch.optim.Adam(model.parameters(), lr=LR, weight_decay=REG), nn.MSELoss()


def fit_data(model, opt, loss_fn, perms, max_steps=None):
    losses = []
    for perm in perms:
        idx = torch.LongTensor(perm)
        num_steps = int(N / 64) - 1
        ep = 0.0
        for mb in range(num_steps if max_steps is None else max_steps):
            i = idx[mb * 64:(mb + 1) * 64]
            opt.zero_grad()
            loss = loss_fn(model(x[i]), y[i])
            loss.backward()
            opt.step()
            ep += loss.detach()
        losses.append(ep.numpy().ravel() / num_steps)
    return losses


fit_data(*host_model(), perm_sets[0], max_steps=50)  # warm-up
model, opt, loss_fn = host_model()
t0 = time.perf_counter()
host_losses = fit_data(model, opt, loss_fn, perm_sets[-1])
host_ms = (time.perf_counter() - t0) * 1e3

ev = sorted(e for e, _ in dev_ms)
lines = [
    f"value-baseline fit, N={N} rows, S={S}, hidden (128, 128), batch 64, {EPOCHS} epochs = {steps} Adam steps",
    f"device ({torch.cuda.get_device_name(0)}): fit_grid, events around the whole fit, {len(ev)} fits after a warm-up: "
    + ", ".join(f"{e:.2f}" for e, _ in dev_ms) + f" ms (median {ev[len(ev) // 2]:.2f} ms, "
    f"{ev[len(ev) // 2] / steps * 1e3:.2f} us per step; host clock until every launch is enqueued: "
    + ", ".join(f"{h:.2f}" for _, h in dev_ms) + " ms)",
    f"host (torch {torch.__version__} CPU, {threads} threads): fit_data loop, one fit: {host_ms:.1f} ms "
    f"({host_ms / steps * 1e3:.1f} us per step)",
    f"ratio host / device: x{host_ms / ev[len(ev) // 2]:.1f}",
    f"epoch losses, same weights and permutations: device {[float(l[0]) for l in dev_out[2]]} "
    f"host {[float(l[0]) for l in host_losses]}; device error_before {float(dev_out[0]):.6f} "
    f"error_after {float(dev_out[1]):.6f}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
