"""Generate tests/golden/g17_bc_fit.npz by running the REFERENCE BC.train.

Dev-container only, like make_golden.py (whose stubs and paths it reuses): imports the
reference from $AMX_REFERENCE (make_golden.py's default) and exits cleanly when it is absent.
No reference source is copied; the fixture holds recorded results only.

G17: mjrl MLP(197, 36, hidden_sizes=(32, 32), seed, init_log_std=-0.25, min_log_std=-2.0)
(mjrl/mjrl/policies/gaussian_mlp.py) warm-started by one BC object
(mjrl/mjrl/algos/behavior_cloning.py, epochs=2, batch_size=64, lr=1e-3) whose train() is
called twice, once per loss type ('MSE', 'MLE'), on seeded synthetic expert paths of 323 rows
(int(323 / 64) = 5 Adam steps per epoch; the second call resumes the optimizer at step 10 and
keeps drawing from the same numpy stream).  The inputs are regenerated from the seeds by the
test (tests/bcfit_ref.py's make_paths, restated here), so only the seeds, the lens, the final
flat parameters, the optimizer state and the logger's loss_before / loss_after are stored.

    python tests/golden/make_golden_bc.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, install_stubs  # noqa: E402

S_BC, A_BC = 197, 36
MODEL_SEED, NUMPY_SEED, PATH_SEED = 1700, 1701, 1702
LENS = (70, 130, 3, 120)  # 323 rows


def g17_paths():
    rs = np.random.RandomState(PATH_SEED)
    Wt = rs.randn(S_BC, A_BC) * 0.05
    paths = []
    for l in LENS:
        obs = rs.randn(l, S_BC)
        act = np.tanh(obs @ Wt) + 0.1 * rs.randn(l, A_BC)
        paths.append(dict(observations=obs, actions=act))
    return paths


def main():
    if not os.path.isdir(REF):
        print(f"{REF} is absent: nothing generated")
        return 0
    install_stubs()
    from mjrl.algos.behavior_cloning import BC
    from mjrl.policies.gaussian_mlp import MLP

    out = {}
    for loss_type in ("MSE", "MLE"):
        pol = MLP(S_BC, A_BC, hidden_sizes=(32, 32), seed=MODEL_SEED, init_log_std=-0.25, min_log_std=-2.0)
        bc = BC(g17_paths(), policy=pol, epochs=2, batch_size=64, lr=1e-3, loss_type=loss_type)
        np.random.seed(NUMPY_SEED)
        bc.train(suppress_fit_tqdm=True)
        bc.train(suppress_fit_tqdm=True)
        k = loss_type.lower()
        out[f"{k}_params"] = pol.get_param_values().astype(np.float32)
        out[f"{k}_loss_before"] = np.array(bc.logger.log["loss_before"], dtype=np.float32)
        out[f"{k}_loss_after"] = np.array(bc.logger.log["loss_after"], dtype=np.float32)
        states = [bc.optimizer.state[p] for p in pol.trainable_params if p in bc.optimizer.state]
        out[f"{k}_step"] = np.int64(int(states[0]["step"]))
        out[f"{k}_n_state"] = np.int64(len(states))
        for i, st in enumerate(states):
            out[f"{k}_exp_avg_{i}"] = st["exp_avg"].numpy()
            out[f"{k}_exp_avg_sq_{i}"] = st["exp_avg_sq"].numpy()
        print(loss_type, "step", out[f"{k}_step"], "states", len(states), "loss_before", out[f"{k}_loss_before"],
              "loss_after", out[f"{k}_loss_after"])
    np.savez_compressed(os.path.join(OUT, "g17_bc_fit.npz"), model_seed=MODEL_SEED, numpy_seed=NUMPY_SEED,
                        path_seed=PATH_SEED, lens=np.array(LENS), **out)
    print("wrote g17_bc_fit.npz")
    return 0


if __name__ == "__main__":
    sys.exit(main())
