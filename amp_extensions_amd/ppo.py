"""The PPO policy update on the device: mjrl's PPO (mjrl/mjrl/algos/ppo_clip.py:23-121) as
run_amp.py:136-140 builds it under --use_ppo.

`PPO` is the drop-in (the reference's constructor, `train_from_paths`, `optimizer`, `logger`,
`running_score`); `DevicePPO` is the engine-level object underneath, beside DeviceNPG: theta in
the reference's flat order and torch.optim.Adam's state in device memory.  One call whitens the
advantages (amx_adv_whiten), scores the old policy (amx_ppo_old_ll), runs the epochs' dependent
batch-64 Adam steps in launches of one workgroup (amx_ppo_steps: csrc/amx_bcfit.hip's step body
with the clipped surrogate's row weights), and takes surr_before / surr_after / kl_dist from
amx_npg_pass' EVAL mode.  The index batches are `plan_bc_batches`: the reference's loop draws
them the same way (ppo_clip.py:90).

The old policy comes in two forms.  "snapshot" is PPO as written: LL_old at the parameters the
call started from.  "tracks_mean" is what the reference computes from its second call on:
MLP.set_param_values (gaussian_mlp.py:75, 87) hands both networks views of one float32 numpy
buffer, so Adam's in-place steps move the old mean network with the new one and only log_std
keeps an old copy.  `PPO` picks the form from the policy's storage before every call.

Same restrictions as the other device learners: the (32, 32) tanh MLP, identity
transformations, mini-batches of 64.
"""
from __future__ import annotations

import time as timer

import numpy as np
import torch

from . import _native as N
from .bc import BATCH, HIDDEN, DataLog, DeviceBC, check_adam, plan_bc_batches, write_optimizer
from .npg import NPG_EVAL, DeviceNPG, engine_rows, pack_policy, paths_to_arrays

OLD_MODES = {"snapshot": N.AMX_PPO_OLD_SNAPSHOT, "tracks_mean": N.AMX_PPO_OLD_TRACKS_MEAN}


class DevicePPO:
    """PPO.train_from_paths for the mjrl Gaussian MLP policy, on the device.

    `policy_layers` / `log_std`: the current policy (nn.Linear layout), also the old one.
    `policy` (optional): a DevicePolicy to refresh after every update.  `old`: "snapshot" or
    "tracks_mean" (an attribute: it may change between calls)."""

    def __init__(self, ctx, policy_layers, log_std, clip_coef=0.2, epochs=10, mb_size=64, learn_rate=3e-4,
                 min_log_std=-3.0, policy=None, old="snapshot", betas=(0.9, 0.999), eps=1e-8):
        if old not in OLD_MODES:
            raise ValueError(f"old must be one of {sorted(OLD_MODES)}, not {old!r}")
        if mb_size != BATCH:
            raise NotImplementedError(f"the device update supports mb_size {BATCH}, not {mb_size}")
        # the EVAL pass (CPI_surrogate, kl_old_new) and the shape checks are DeviceNPG's
        self._npg = DeviceNPG(ctx, policy_layers, log_std, min_log_std=min_log_std)
        # theta and the Adam state of all seven tensors are DeviceBC's under MLE
        self._bc = DeviceBC(ctx, pack_policy(policy_layers, log_std), lr=learn_rate, betas=betas, eps=eps,
                            loss_type="MLE")
        self.ctx, self.S, self.A, self.P = ctx, ctx.S, ctx.A, self._bc.P
        self.lr, self.betas, self.eps = float(learn_rate), (float(betas[0]), float(betas[1])), float(eps)
        self.theta = self._bc.theta  # updated in place, never rebound
        self.theta_old = self.theta.clone()
        self.clip_coef, self.epochs, self.old = float(clip_coef), int(epochs), old
        self.min_log_std = float(min_log_std)
        self.policy = policy
        self._losses = self._clipped = None

    # ---- parameters (reference flat order) --------------------------------------------------------

    def get_param_values(self) -> np.ndarray:
        return self.theta.cpu().numpy().copy()

    def set_param_values(self, new_params) -> None:
        """MLP.set_param_values with set_new and set_old (gaussian_mlp.py:69-91): float32, log_std
        clamped at min_log_std."""
        t = new_params.detach() if isinstance(new_params, torch.Tensor) else torch.from_numpy(np.asarray(new_params))
        if t.numel() != self.P:
            raise ValueError(f"the vector holds {t.numel()} values, the policy has {self.P}")
        t = t.reshape(-1).to(self.ctx.device, torch.float32).clone()
        t[-self.A:].clamp_(min=self.min_log_std)
        self.theta.copy_(t)
        self.theta_old.copy_(t)
        self._sync_policy()

    def _sync_policy(self) -> None:
        if self.policy is not None:
            self._npg.theta = self.theta
            self.policy.sync_from(*self._npg._layers_view())

    @property
    def step_losses(self) -> np.ndarray:
        """The last call's fp32 loss of every step."""
        return np.zeros(0, dtype=np.float32) if self._losses is None else self._losses.cpu().numpy()

    @property
    def step_clipped(self) -> np.ndarray:
        """The last call's rows (of 64) with LR outside [1 - c, 1 + c], per step."""
        return np.zeros(0, dtype=np.int32) if self._clipped is None else self._clipped.cpu().numpy()

    # ---- Adam state (DeviceBC's surface) ---------------------------------------------------------

    def load_optimizer(self, optimizer) -> None:
        """Adam state of a torch.optim.Adam over the policy's trainable_params -> the device."""
        self._bc.load_optimizer(optimizer)

    def adam_state(self):
        """(step, [exp_avg per parameter], [exp_avg_sq per parameter]) on the host."""
        return self._bc.adam_state()

    # ---- the update -------------------------------------------------------------------------------

    def _eval(self, old, new, obs, act, adv, out) -> None:
        """out[0:2] = sums over the rows of exp(LL_new - LL_old) adv and of the mean_kl terms."""
        self._npg.theta = old
        self._npg._pass(NPG_EVAL, obs, act, adv, new, out=out)

    def train_from_arrays(self, observations, actions, advantages, batches=None,
                          max_steps_per_launch: int = 2048) -> dict:
        """PPO.train_from_paths on concatenated arrays (ppo_clip.py:58-103).  `batches`: int
        [epochs][int(N / 64)][64] row indices (default: plan_bc_batches from numpy's global
        generator).  The steps run in launches of at most `max_steps_per_launch`; the cut
        changes no bit.  Leaves theta with log_std clamped at min_log_std and the old policy
        equal to it, as the reference's write-back does.  Returns surr_before, surr_after,
        kl_dist (of the parameters before the clamp, as the reference scores them) and the
        whitened advantages."""
        c, dev, A = self.ctx, self.ctx.device, self.A
        if self.old not in OLD_MODES:
            raise ValueError(f"old must be one of {sorted(OLD_MODES)}, not {self.old!r}")
        if max_steps_per_launch < 1:
            raise ValueError("max_steps_per_launch must be positive")
        obs, act, adv = self._npg._inputs(observations, actions, advantages)  # fp32 rows, once
        n = obs.shape[0]
        steps = int(n / BATCH)
        if batches is None:
            batches = plan_bc_batches(n, self.epochs)
        idx = np.ascontiguousarray(np.asarray(batches).reshape(-1, BATCH), dtype=np.int32)
        if idx.shape[0] != self.epochs * steps:
            raise ValueError(f"batches hold {idx.shape[0]} steps, {self.epochs} epochs of {steps} are due")
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"batches must hold row indices in [0, {n})")
        total = idx.shape[0]
        adv = self._npg._whiten(adv)  # (adv - mean) / (std + 1e-6), population std, in fp64
        adv32 = adv.to(torch.float32)
        tracks = self.old == "tracks_mean"
        ls_old = self.theta_old[-A:].clone()
        old0 = torch.cat([self.theta[:-A], ls_old]) if tracks else self.theta_old.clone()
        res = torch.empty(4, dtype=torch.float64, device=dev)  # surr_before, kl | surr_after, kl
        self._eval(old0, self.theta, obs, act, adv, res[0:2])
        self._losses = torch.zeros(total, dtype=torch.float32, device=dev)
        self._clipped = torch.zeros(total, dtype=torch.int32, device=dev)
        if total:
            ll_old = None
            if not tracks:
                ll_old = torch.empty(n, dtype=torch.float32, device=dev)
                N.check(c.lib.amx_ppo_old_ll(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                             self.theta_old.data_ptr(), ll_old.data_ptr(), c.stream), "amx_ppo_old_ll")
            m, v, step = self._bc._adam_state()
            idx_d = torch.from_numpy(idx).to(dev)
            b1, b2 = self.betas
            for k0 in range(0, total, max_steps_per_launch):
                k = min(max_steps_per_launch, total - k0)
                N.check(c.lib.amx_ppo_steps(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                            adv32.data_ptr(), N.ptr(ll_old), ls_old.data_ptr(), OLD_MODES[self.old],
                                            idx_d[k0:].data_ptr(), k, self.theta.data_ptr(), m.data_ptr(),
                                            v.data_ptr(), step.data_ptr(), self.lr, b1, b2, self.eps, self.clip_coef,
                                            self._losses[k0:].data_ptr(), self._clipped[k0:].data_ptr(), c.stream),
                        "amx_ppo_steps")
        old1 = torch.cat([self.theta[:-A], ls_old]) if tracks else old0
        self._eval(old1, self.theta, obs, act, adv, res[2:4])
        self.theta[-A:].clamp_(min=self.min_log_std)
        self.theta_old.copy_(self.theta)
        self._sync_policy()
        sb, _, sa, kl = res.tolist()  # the call's one host sync
        return {"surr_before": sb / n, "surr_after": sa / n, "kl_dist": kl / n, "advantages": adv}

    def train_from_paths(self, paths, infos: dict | None = None):
        """Reference surface: mjrl path dicts (observations, actions, advantages, rewards) ->
        base_stats [mean, std, min, max] of the path returns; infos updated with the call's results."""
        obs, act, adv, base_stats = paths_to_arrays(paths)
        out = self.train_from_arrays(obs, act, adv)
        if infos is not None:
            infos.update(out)
        return base_stats

    def train_from_engine(self, engine, advantages: torch.Tensor, **kw) -> dict:
        """Update from the rollout engine's buffers without a host round trip: the recorded
        transitions obs[:T], acts[:T] ([T, B] rows) and GAE advantages [T, B]."""
        return self.train_from_arrays(*engine_rows(engine, advantages, self.S, self.A), **kw)


def _shared_storage(policy) -> bool:
    """Whether policy.old_model's six tensors are policy.model's (the state MLP.set_param_values
    leaves behind: gaussian_mlp.py:75, 87 slice one float32 buffer for both)."""
    same = [p.data_ptr() == q.data_ptr() for p, q in zip(policy.model.parameters(), policy.old_model.parameters())]
    if all(same):
        return True
    if any(same):
        raise NotImplementedError("policy.old_model shares some tensors with policy.model and not others")
    return False


class PPO:
    """mjrl's PPO (ppo_clip.py:23-121) with the update on the device.  `policy`: an mjrl MLP or
    any object with its attribute layout (model / old_model with fc_layers, log_std / old_log_std,
    trainable_params / old_params, get_param_values, set_param_values, min_log_std).  `ctx`: the
    AmxContext to run on (one is made for the policy's sizes when None).  train_step and the
    rollout statistics come from the reference's BatchREINFORCE, e.g.
    `class PPO(amx.PPO, BatchREINFORCE): pass`."""

    def __init__(self, env, policy, baseline, clip_coef=0.2, epochs=10, mb_size=64, learn_rate=3e-4, seed=123,
                 save_logs=False, ctx=None, **kwargs):
        tr = getattr(policy.model, "transformations", None)
        if tr and any(x is not None for x in tr.values()):
            raise NotImplementedError("the policy's model has input / output transformations: the device policy "
                                      "assumes identity transformations")
        hidden = tuple(l.weight.shape[0] for l in list(policy.model.fc_layers)[:-1])
        if hidden != HIDDEN:
            raise NotImplementedError(f"the device update supports hidden sizes {HIDDEN}, not {hidden}")
        if mb_size != BATCH:
            raise NotImplementedError(f"the device update supports mb_size {BATCH}, not {mb_size}")
        self.env = env
        self.policy = policy
        self.baseline = baseline
        self.learn_rate = learn_rate
        self.seed = seed
        self.save_logs = save_logs
        self.clip_coef = clip_coef
        self.epochs = epochs
        self.mb_size = mb_size
        self.running_score = None
        self.ctx = ctx
        self.device_ppo = None
        self.logger = DataLog()
        self.optimizer = torch.optim.Adam(self.policy.trainable_params, lr=learn_rate)

    def _device_ppo(self) -> DevicePPO:
        """The engine object, built on first use; the optimizer's current hyper-parameters."""
        pol = self.policy
        layers = [(l.weight, l.bias) for l in pol.model.fc_layers]
        S, A = layers[0][0].shape[1], layers[-1][0].shape[0]
        if self.ctx is None:
            from .engine import AmxContext
            self.ctx = AmxContext(S, A)
        if (self.ctx.S, self.ctx.A) != (S, A):
            raise ValueError("the policy's sizes do not match the context's S, A")
        if self.device_ppo is None:
            self.device_ppo = DevicePPO(self.ctx, layers, pol.log_std, mb_size=self.mb_size,
                                        min_log_std=float(pol.min_log_std))
        d, g = self.device_ppo, self.optimizer.param_groups[0]
        d.lr, d.betas, d.eps = float(g["lr"]), tuple(map(float, g["betas"])), float(g["eps"])
        d.clip_coef, d.epochs = float(self.clip_coef), int(self.epochs)
        return d

    def train_from_paths(self, paths):
        check_adam(self.optimizer)
        if self.optimizer.param_groups[0]["weight_decay"]:
            raise NotImplementedError("the device update implements Adam without weight decay")
        if self.mb_size != BATCH:
            raise NotImplementedError(f"the device update supports mb_size {BATCH}, not {self.mb_size}")
        tracks = _shared_storage(self.policy)

        observations = np.concatenate([path["observations"] for path in paths])
        actions = np.concatenate([path["actions"] for path in paths])
        advantages = np.concatenate([path["advantages"] for path in paths])

        path_returns = [sum(p["rewards"]) for p in paths]
        mean_return = np.mean(path_returns)
        base_stats = [mean_return, np.std(path_returns), np.amin(path_returns), np.amax(path_returns)]
        self.running_score = mean_return if self.running_score is None else \
            0.9 * self.running_score + 0.1 * mean_return
        if self.save_logs and hasattr(self, "log_rollout_statistics"):
            self.log_rollout_statistics(paths)

        ts = timer.time()
        d = self._device_ppo()
        d.old = "tracks_mean" if tracks else "snapshot"
        # as the policy holds them (no clamp here: the reference's loop reads them as they are)
        d.theta.copy_(torch.from_numpy(self.policy.get_param_values()))
        d.theta_old.copy_(torch.cat([p.data.reshape(-1).float() for p in self.policy.old_params]))
        d.load_optimizer(self.optimizer)
        out = d.train_from_arrays(observations, actions, advantages)
        write_optimizer(self.optimizer, d._bc)  # all seven tensors: DeviceBC under MLE
        self.policy.set_param_values(d.theta.cpu().numpy(), set_new=True, set_old=True)
        t_opt = timer.time() - ts

        if self.save_logs:
            self.logger.log_kv('t_opt', t_opt)
            self.logger.log_kv('kl_dist', np.float32(out["kl_dist"]))
            self.logger.log_kv('surr_improvement', np.float32(out["surr_after"] - out["surr_before"]))
            self.logger.log_kv('running_score', self.running_score)
            try:
                self.env.env.env.evaluate_success(paths, self.logger)
            except Exception:
                try:
                    self.logger.log_kv('success_rate', self.env.env.env.evaluate_success(paths))
                except Exception:
                    pass
        return base_stats
