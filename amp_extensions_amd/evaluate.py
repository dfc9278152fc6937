"""`evaluate` drop-in (milo/milo/utils.py:115-217) on the learned-dynamics env.

The reference evaluates a policy in the real DeepMimic env: `num_traj` greedy and `num_traj`
sampled trajectories, scored by the env's `dtw_cost` (imitate_amp) or the reward sums, plus the
MMD of their cost inputs to the expert's (or the mean GAIL cost), logged and written to the
TensorBoard writer under the reference's tags.  Here `env` is the model-based env (a
BatchedSimEnv or RolloutEngine on a ReferenceMotion): the two `sample_points` calls run on the
device and deliver `dtw_cost` through a dtw.TimeWarper, so run.py:238 binds this function by
import with `mb_env`.  Signature, log lines, writer tags and the returned (scores, costs) are
the reference's.
"""
from __future__ import annotations

import numpy as np
import torch

from .dtw import TimeWarper
from .sampler import sample_points
from .sim_env import BatchedSimEnv


def time_warper(env, update_rate: float = 30.0, time_end_max: float = 10.0) -> TimeWarper:
    """The env's TimeWarper (cached on its engine): `env.dtw` when the caller set one."""
    own = getattr(env, "dtw", None)
    if own is not None:
        return own
    src = env.engine if isinstance(env, BatchedSimEnv) else env
    if getattr(src, "motion", None) is None:
        raise ValueError("evaluate(imitate_amp=True) needs an env reset from a ReferenceMotion (the DTW score aligns "
                         "with the clip)")
    cache = src.__dict__.setdefault("_time_warpers", {})
    key = (float(update_rate), float(time_end_max))
    if key not in cache:
        cache[key] = TimeWarper(src.ctx, src.motion, update_rate, time_end_max)
    return cache[key]


def _cost_inputs(paths, input_type: str) -> torch.Tensor:
    second = {"sa": "actions", "ss": "next_observations"}[input_type]
    x = np.concatenate([np.concatenate([p["observations"], p[second]], axis=1) for p in paths], axis=0)
    return torch.from_numpy(x).float()


def evaluate(n_iter, logger, writer, args, env, policy, reward_func, num_traj=10, imitate_amp=True, gail_cost=False):
    """utils.py:115-217.  Returns ({'greedy', 'sample'} mean scores, {'greedy', 'sample'} MMD or
    mean GAIL cost)."""
    seed = args.seed + n_iter
    logger.info(f"=== Evaluating with seed: {seed} ===")
    dtw = time_warper(env) if imitate_amp else None
    runs = {}
    for name, greedy in (("greedy", True), ("sample", False)):
        paths = sample_points(env=env, policy=policy, num_to_collect=num_traj, base_seed=seed,
                              num_workers=args.num_cpu, mode="trajectories", eval_mode=greedy, verbose=False,
                              deepmimic=True, dtw=dtw)
        if imitate_amp:
            score = np.array([p["env_infos"][-1]["dtw_cost"] for p in paths])
        else:
            score = np.array([np.sum(p["rewards"]) for p in paths])
        r = dict(score=score, length=np.mean([len(p["rewards"]) for p in paths]))
        if reward_func is None:
            r["cost"] = 0.0
        else:
            x = _cost_inputs(paths, args.cost_input_type)
            if gail_cost:
                r["cost"] = reward_func.get_costs(x).mean()
            else:
                diff = reward_func.get_rep(x).mean(0) - reward_func.phi_e
                r["cost"] = torch.dot(diff, diff)
        runs[name] = r
    if reward_func is None:
        print("Not caring about MMD here -- doing model-based RL")

    score_log = "DTW Cost" if imitate_amp else "Reward"
    score_tag = "dtw_cost" if imitate_amp else "reward"
    cost_log = "GAIL cost" if gail_cost else "MMD"
    cost_tag = "gail_cost" if gail_cost else "mmd"
    for name, title in (("greedy", "Greedy"), ("sample", "Sampled")):
        r = runs[name]
        s = r["score"]
        logger.info(f"{title} Evaluation {score_log} mean (min, max): {s.mean():.2f} ({s.min():.2f}, {s.max():.2f})")
        logger.info(f"{title} Evaluation Trajectory Lengths: {r['length']:.2f}")
        logger.info(f"{title} {cost_log}: {r['cost']}")
    for name, tag in (("greedy", "greedy"), ("sample", "sampled")):
        r = runs[name]
        s = r["score"]
        writer.add_scalars(f"data/inf_{tag}_{score_tag}",
                           {"min_score": s.min(), "mean_score": s.mean(), "max_score": s.max()}, n_iter + 1)
        writer.add_scalar(f"data/inf_{tag}_len", r["length"], n_iter + 1)
        writer.add_scalar(f"data/{tag}_{cost_tag}", r["cost"], n_iter + 1)
    scores = {name: runs[name]["score"].mean() for name in ("greedy", "sample")}
    costs = {name: runs[name]["cost"] for name in ("greedy", "sample")}
    return scores, costs
