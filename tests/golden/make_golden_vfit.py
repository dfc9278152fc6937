"""Generate tests/golden/g14_baseline_fit.npz by running the REFERENCE MLPBaseline.fit.

Dev-container only, like make_golden.py (whose stubs and paths it reuses): imports the
reference from $AMX_REFERENCE (make_golden.py's default) and exits cleanly when it is absent.
No reference source is copied; the fixture holds recorded results only.

G14: mjrl MLPBaseline(inp_dim=226, reg_coef=1e-3, batch_size=64, epochs=2, learn_rate=1e-3)
(mjrl/mjrl/baselines/mlp_baseline.py) fitted twice in a row on seeded synthetic paths of 400
rows each (int(400 / 64) - 1 = 5 Adam steps per epoch; the second call resumes the optimizer
at step 10 and keeps drawing from the same numpy stream).  The inputs are regenerated from
the seeds by the test (`g14_paths`, restated there), so only the seeds, the three return
values of each call, the final weights and the optimizer state are stored.

    python tests/golden/make_golden_vfit.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, S, install_stubs  # noqa: E402

MODEL_SEED, NUMPY_SEED, PATH_SEEDS = 1400, 1401, (1402, 1403)
LENS = (40, 75, 3, 120, 64, 98)  # 400 rows


def g14_paths(seed):
    """Ragged synthetic paths: observations partly beyond the +-10 clip, float64 returns."""
    rs = np.random.RandomState(seed)
    paths = []
    for l in LENS:
        obs = rs.randn(l, S) * 4.0
        obs[:, 3] *= 6.0
        paths.append(dict(observations=obs, rewards=np.zeros(l, dtype=np.float32), returns=rs.randn(l) * 2.0 + 1.0))
    return paths


def main():
    if not os.path.isdir(REF):
        print(f"{REF} is absent: nothing generated")
        return 0
    install_stubs()
    from mjrl.baselines.mlp_baseline import MLPBaseline

    torch.manual_seed(MODEL_SEED)
    bl = MLPBaseline(inp_dim=S, reg_coef=1e-3, batch_size=64, epochs=2, learn_rate=1e-3)
    out = {}
    np.random.seed(NUMPY_SEED)
    for call, seed in enumerate(PATH_SEEDS):
        eb, ea, losses = bl.fit(g14_paths(seed), return_errors=True, return_all_errors=True)
        out[f"error_before_{call}"] = np.float32(eb)
        out[f"error_after_{call}"] = np.float32(ea)
        out[f"epoch_losses_{call}"] = np.concatenate(losses).astype(np.float32)
    for k, v in bl.model.state_dict().items():
        out["model." + k] = v.numpy()
    params = bl.optimizer.param_groups[0]["params"]
    for i, p in enumerate(params):
        st = bl.optimizer.state[p]
        out[f"exp_avg_{i}"] = st["exp_avg"].numpy()
        out[f"exp_avg_sq_{i}"] = st["exp_avg_sq"].numpy()
    out["step"] = np.int64(int(bl.optimizer.state[params[0]]["step"]))
    np.savez_compressed(os.path.join(OUT, "g14_baseline_fit.npz"), model_seed=MODEL_SEED, numpy_seed=NUMPY_SEED,
                        path_seeds=np.array(PATH_SEEDS), lens=np.array(LENS), **out)
    print("wrote g14_baseline_fit.npz: step", out["step"], "errors",
          [float(out[f"error_{w}_{c}"]) for c in (0, 1) for w in ("before", "after")])
    return 0


if __name__ == "__main__":
    sys.exit(main())
