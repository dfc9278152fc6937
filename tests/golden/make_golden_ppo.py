"""Generate tests/golden/g20_ppo_update.npz by running the REFERENCE PPO.train_from_paths.

Dev-container only, like make_golden.py (whose stubs and paths it reuses): imports the
reference from $AMX_REFERENCE (make_golden.py's default) and exits cleanly when it is absent.
No reference source is copied; the fixture holds recorded results and seeds only.

G20: mjrl MLP(197, 36, hidden_sizes=(32, 32), seed=123, init_log_std=-0.25, min_log_std=m)
(mjrl/mjrl/policies/gaussian_mlp.py) updated by one PPO object (mjrl/mjrl/algos/ppo_clip.py,
epochs=2, mb_size=64) whose train_from_paths is called twice on seeded synthetic paths of 323
rows (int(323 / 64) = 5 Adam steps per epoch; the second call resumes the optimizer at step 10,
keeps drawing from the same numpy stream and runs with old_model's tensors sharing model's
storage).  Two variants: `default` (learn_rate 3e-4, m = -0.2515, np.random.seed(77)) and
`clipped` (learn_rate 3e-3, m = -0.26, np.random.seed(84)).  The inputs are regenerated from the
seeds by the tests (tests/ppo_ref.py's make_paths, restated here).

    python tests/golden/make_golden_ppo.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, install_stubs  # noqa: E402

S_PPO, A_PPO = 197, 36
MODEL_SEED, PATH_SEED = 123, 5
LENS = (70, 130, 3, 120)  # 323 rows
VARIANTS = {"default": dict(learn_rate=3e-4, min_log_std=-0.2515, numpy_seed=77),
            "clipped": dict(learn_rate=3e-3, min_log_std=-0.26, numpy_seed=84)}


def g20_paths(policy):
    import torch
    rs = np.random.RandomState(PATH_SEED)
    paths = []
    for l in LENS:
        obs = rs.randn(l, S_PPO)
        adv = rs.randn(l) * 2 + 0.3
        rew = rs.randn(l)
        paths.append(dict(observations=obs, advantages=adv, rewards=rew))
    for p in paths:
        with torch.no_grad():
            mean = policy.model(torch.from_numpy(p["observations"]).float()).numpy()
        p["actions"] = np.float64(mean + np.exp(-0.25) * rs.randn(len(mean), A_PPO))
    return paths


def main():
    if not os.path.isdir(REF):
        print(f"{REF} is absent: nothing generated")
        return 0
    install_stubs()
    from mjrl.algos.ppo_clip import PPO
    from mjrl.policies.gaussian_mlp import MLP

    out = {}
    for k, var in VARIANTS.items():
        pol = MLP(S_PPO, A_PPO, hidden_sizes=(32, 32), seed=MODEL_SEED, init_log_std=-0.25,
                  min_log_std=var["min_log_std"])
        paths = g20_paths(pol)
        ppo = PPO(None, pol, None, epochs=2, mb_size=64, learn_rate=var["learn_rate"], save_logs=True)
        ppo.log_rollout_statistics = lambda paths: None  # BatchREINFORCE's needs an env
        np.random.seed(var["numpy_seed"])
        shared = []
        for call in range(2):
            shared.append(all(p.data_ptr() == q.data_ptr()
                              for p, q in zip(pol.model.parameters(), pol.old_model.parameters())))
            out[f"{k}_base_stats"] = np.array(ppo.train_from_paths(paths), dtype=np.float64)
            out[f"{k}_params_{call}"] = pol.get_param_values().astype(np.float32)
        assert shared == [False, True], shared
        out[f"{k}_kl_dist"] = np.array(ppo.logger.log["kl_dist"], dtype=np.float32)
        out[f"{k}_surr_improvement"] = np.array(ppo.logger.log["surr_improvement"], dtype=np.float32)
        out[f"{k}_running_score"] = np.float64(ppo.running_score)
        states = [ppo.optimizer.state[p] for p in pol.trainable_params]
        out[f"{k}_step"] = np.int64(int(states[0]["step"]))
        for i, st in enumerate(states):
            out[f"{k}_exp_avg_{i}"] = st["exp_avg"].numpy()
            out[f"{k}_exp_avg_sq_{i}"] = st["exp_avg_sq"].numpy()
        out[f"{k}_learn_rate"] = np.float64(var["learn_rate"])
        out[f"{k}_min_log_std"] = np.float64(var["min_log_std"])
        out[f"{k}_numpy_seed"] = np.int64(var["numpy_seed"])
        print(k, "step", out[f"{k}_step"], "kl_dist", out[f"{k}_kl_dist"], "surr_improvement",
              out[f"{k}_surr_improvement"])
    np.savez_compressed(os.path.join(OUT, "g20_ppo_update.npz"), model_seed=MODEL_SEED, path_seed=PATH_SEED,
                        lens=np.array(LENS), **out)
    print("wrote g20_ppo_update.npz")
    return 0


if __name__ == "__main__":
    sys.exit(main())
