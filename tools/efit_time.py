"""Time the device ensemble training (DeviceEnsemble.fit_epoch: amx_efit_step per mini-batch,
csrc/amx_efit.hip) at the README command's shape -- 4 members, hidden [512] x 4, S/A 197/36,
batch 256 -- on 20 480 synthetic rows, 2 epochs of Adam with grad_clip=1, against the
reference loop restated in torch (tests/efit_ref.py, the tests' comparator, fp32) on the same
box's CPU threads.

The device epochs are timed with events around whole epochs (index upload, every step's
launches, the loss read-back), after a warm-up epoch; both sides start from the same weights
and take the same index batches, and their epoch losses are printed side by side.

usage: python tools/efit_time.py [out.txt] [cpu_threads] [--no-host] [--plain] [--forward]
(--no-host: the device part only, for a kernel-trace run of its own; --plain: run.py's default
model instead -- plain members, dense_connect=False, hidden [1024, 1024] -- through
PlainDynamicsEnsemble and tests/plain_ref.py, plus the f16x3 inference forward of 256 lanes timed
in-kernel, AmxContext.gemm_timer; --forward: that forward line for the dense-connect shape too)
"""
import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amp_extensions_amd.datasets import AmpDataset  # noqa: E402
from amp_extensions_amd.ensemble import (DynamicsEnsemble, PlainDynamicsEnsemble, index_loader, materialise,  # noqa: E402
                                         plan_batches)
from efit_ref import events_from_plan, restate_member, synthetic_transitions  # noqa: E402
from plain_ref import restate_member as restate_plain_member  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
no_host = "--no-host" in sys.argv
plain = "--plain" in sys.argv
out_path = args[0] if args else os.path.join("profiles", "efit_time_plain.txt" if plain else "efit_time.txt")
threads = int(args[1]) if len(args) > 1 else 16
S, A, HIDDEN, M, BATCH, N, EPOCHS, CLIP = 197, 36, [512] * 4, 4, 256, 20480, 2, 1.0
if plain:
    HIDDEN, DynamicsEnsemble, restate_member = [1024, 1024], PlainDynamicsEnsemble, restate_plain_member
OPT = {"optim": "adam", "lr": 1e-3, "eps": 1e-8}
steps = -(-N // BATCH)

tr = synthetic_transitions(N, S, A, 0)
ens = DynamicsEnsemble(S, A, AmpDataset(*tr), None, num_models=M, batch_size=BATCH, hidden_sizes=HIDDEN,
                       optim_args=OPT, device=torch.device("cpu"))
init = [(copy.deepcopy(m.model.state_dict())) for m in ens.models]
torch.manual_seed(0)
plan, _ = plan_batches(N, 0, BATCH, EPOCHS + 1, M, False)  # epoch 0 of the plan is the warm-up's
loader = index_loader(N, BATCH)


def epoch_indices(e):
    per = [materialise(loader, plan[g][e][0]) for g in range(M)]
    idx = np.zeros((M, steps, BATCH), dtype=np.int32)
    for g in range(M):
        for s, b in enumerate(per[g]):
            idx[g, s, :len(b)] = b
    return idx, [len(b) for b in per[0]]


eng = ens.engine
eng.fit_begin(tr, "adam", OPT["lr"], OPT["eps"], BATCH)
eng.fit_epoch(*epoch_indices(0), train=True, grad_clip=CLIP)  # warm-up: code objects
eng.set_weights([m.model.layers() for m in ens.models])  # back to the initial weights, fresh optimizer
eng.fit_end()
eng.fit_begin(tr, "adam", OPT["lr"], OPT["eps"], BATCH)
torch.cuda.synchronize()
dev_ms, dev_loss = [], []
for e in range(1, EPOCHS + 1):
    idx, sizes = epoch_indices(e)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    losses = eng.fit_epoch(idx, sizes, train=True, grad_clip=CLIP)
    e1.record()
    torch.cuda.synchronize()
    dev_ms.append(e0.elapsed_time(e1))
    dev_loss.append([float(np.average([float(x) for x in losses[g]])) for g in range(M)])
eng.fit_end()
dev_total = sum(dev_ms)


def forward_us(e, reps=200):
    """Mean in-kernel time of the f16x3 forward of BATCH lanes (first hidden layer's start to the
    output layer's last workgroup, AmxContext.gemm_timer), after a warm-up."""
    ob, ac = tr[0][:BATCH].cuda(), tr[1][:BATCH].cuda()
    for _ in range(10):
        e.forward_preds(ob, ac, BATCH)
    timer = e.ctx.gemm_timer()
    for _ in range(reps):
        e.forward_preds(ob, ac, BATCH)
    torch.cuda.synchronize()
    t = timer.cpu().tolist()
    e.ctx.gemm_timer(False)
    assert t[3] == reps, t
    return t[2] / t[3] / 100.0  # 100 MHz ticks


lines = [
    f"ensemble training, {M} {'plain' if plain else 'dense-connect'} members, hidden {HIDDEN}, S/A {S}/{A}, "
    f"batch {BATCH}, {N} rows: {EPOCHS} epochs x "
    f"{steps} steps of Adam, grad_clip {CLIP}",
    f"device ({torch.cuda.get_device_name(0)}): fit_epoch, events around whole epochs after a warm-up epoch: "
    + ", ".join(f"{x:.1f}" for x in dev_ms) + f" ms; {dev_total / (EPOCHS * steps) * 1e3:.1f} us per step "
    f"(all {M} members)",
]
if plain or "--forward" in sys.argv:
    lines.append(f"f16x3 inference forward, {BATCH} lanes x {M} members, in-kernel (gemm_timer, mean of 200): "
                 f"{forward_us(eng):.1f} us")
if not no_host:
    torch.set_num_threads(threads)
    data = {"train": tr}
    norms = ens.transformations
    ev = [events_from_plan(plan[g][1:], loader, None, materialise) for g in range(M)]
    restate_member(init[0], None, norms, data, ev[0][:3], "adam", OPT["lr"], OPT["eps"], CLIP, torch.float32)  # warm-up
    t0 = time.perf_counter()
    host = [restate_member(init[g], None, norms, data, ev[g], "adam", OPT["lr"], OPT["eps"], CLIP, torch.float32)
            for g in range(M)]
    host_ms = (time.perf_counter() - t0) * 1e3
    host_loss = [[float(np.average([l for _, l in host[g]["losses"]][e * steps:(e + 1) * steps])) for g in range(M)]
                 for e in range(EPOCHS)]
    lines += [
        f"host (torch {torch.__version__} CPU, {threads} threads, fp32): the restated loop, member after member, "
        f"{EPOCHS} epochs: {host_ms:.0f} ms ({host_ms / (EPOCHS * steps) * 1e3:.0f} us per step of all {M} members)",
        f"ratio host / device: x{host_ms / dev_total:.1f}",
        f"epoch losses per member, same weights and batches: device {np.round(dev_loss, 6).tolist()} "
        f"host {np.round(host_loss, 6).tolist()}",
    ]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
