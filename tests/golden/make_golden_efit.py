"""Generate tests/golden/g15_ensemble_train.npz by running the REFERENCE's own
DynamicsEnsemble.train (milo/milo/dynamics.py:82-108, 305-378).

Dev-container only; reuses make_golden.py's stubs and exits cleanly without the reference.
The fixture holds results only (the inputs are regenerated from seeds by the test,
tests/efit_ref.py:synthetic_transitions).

Two blocks at S/A = 24/6, hidden [32, 32], 4 members, batch 256, 600 train rows (batches of
256, 256, 88) and 300 validation rows, epochs=2, validate=True, torch.manual_seed right
before train:
  adam  run.py's optimizer defaults (Adam, lr 1e-3, eps 1e-8), grad_clip=1.0
  sgd   SGD-Nesterov at an lr large enough that epoch 2's train loss exceeds epoch 1's for a
        member (best epoch != last epoch): pins that train() ends with the LAST epoch's
        parameters (on current torch its "best" dicts are state_dict() views of the live
        tensors).  The lr sits just under the blow-up, and the seeds of both blocks are ones
        for which the fp32 reference stays within a quarter of the test's tolerance of an fp64
        restatement (larger rates amplify rounding beyond it).
Recorded per block: the returned (train_min_loss, train_losses[0]) pairs, every member's final
weights, the optimizer state and the step count.

Usage:  python tests/golden/make_golden_efit.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
from efit_ref import synthetic_transitions  # noqa: E402

S, A, HIDDEN, M, BATCH = 24, 6, [32, 32], 4, 256
N_TRAIN, N_VAL, SEED_TRAIN, SEED_VAL, EPOCHS = 600, 300, 15, 16, 2
BLOCKS = {
    "adam": dict(optim_args={"optim": "adam", "lr": 1e-3, "eps": 1e-8}, grad_clip=1.0, seed=1507),
    "sgd": dict(optim_args={"optim": "sgd", "lr": 4.5, "momentum": 0.9}, grad_clip=0.0, seed=1508),
}


def run_block(name, cfg):
    from milo.datasets import AmpDataset
    from milo.dynamics import DynamicsEnsemble
    tr = AmpDataset(*synthetic_transitions(N_TRAIN, S, A, SEED_TRAIN))
    va = AmpDataset(*synthetic_transitions(N_VAL, S, A, SEED_VAL))
    ens = DynamicsEnsemble(S, A, tr, va, num_models=M, batch_size=BATCH, hidden_sizes=HIDDEN, transform=True,
                           dense_connect=True, optim_args=cfg["optim_args"], base_seed=100,
                           device=torch.device("cpu"))
    torch.manual_seed(cfg["seed"])
    info = ens.train(EPOCHS, validate=True, grad_clip=cfg["grad_clip"])
    out = {f"{name}_info": np.array(info, dtype=np.float64), f"{name}_seed": cfg["seed"],
           f"{name}_grad_clip": cfg["grad_clip"], f"{name}_lr": cfg["optim_args"]["lr"],
           f"{name}_p1": cfg["optim_args"].get("eps", cfg["optim_args"].get("momentum"))}
    for k, m in enumerate(ens.models):
        params = list(m.model.parameters())
        for j, p in enumerate(params):
            tag = f"{name}_m{k}_p{j}"
            out[tag] = p.detach().numpy().copy()
            st = m.optimizer.state[p]
            if name == "adam":
                out[tag + "_exp_avg"] = st["exp_avg"].numpy().copy()
                out[tag + "_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
                out[f"{name}_m{k}_step"] = np.float64(float(st["step"]))
            else:
                out[tag + "_buf"] = st["momentum_buffer"].numpy().copy()
    return out


def main():
    if not os.path.isdir(os.path.join(MG.REF, "milo")):
        print(f"[make_golden_efit] {MG.REF} not present: nothing to do")
        return 0
    MG.install_stubs()
    torch.set_num_threads(1)
    out = dict(S=S, A=A, hidden=np.array(HIDDEN), M=M, batch=BATCH, n_train=N_TRAIN, n_val=N_VAL,
               seed_train=SEED_TRAIN, seed_val=SEED_VAL, epochs=EPOCHS)
    for name, cfg in BLOCKS.items():
        out.update(run_block(name, cfg))
    info = out["sgd_info"]
    assert np.isfinite(info).all() and (info[:, 0] == info[:, 1]).any(), \
        f"sgd block: epoch 2's train loss must exceed epoch 1's for a member, got {info}"
    assert (out["adam_info"][:, 0] < out["adam_info"][:, 1]).all(), out["adam_info"]
    assert all(np.isfinite(v).all() for v in out.values() if isinstance(v, np.ndarray))
    path = os.path.join(HERE, "g15_ensemble_train.npz")
    np.savez_compressed(path, **out)
    print("[make_golden_efit] wrote", path, os.path.getsize(path), "bytes")
    print("adam", out["adam_info"].tolist())
    print("sgd", info.tolist())
    return 0


if __name__ == "__main__":
    sys.exit(main())
