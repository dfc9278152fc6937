"""The behaviour-cloning warm start on the device: mjrl's BC
(mjrl/mjrl/algos/behavior_cloning.py:14-145) as run.py:202-211 uses it before the first
policy-gradient step.

`BC` is the drop-in (the reference's constructor, `train` / `fit`, `optimizer`, `logger`);
`DeviceBC` is the engine-level object underneath: theta in the reference's flat order
(DeviceNPG.theta's layout) and the Adam state in device memory, trained by `amx_bcfit_steps`
(csrc/amx_bcfit.hip: a whole run of dependent mini-batch steps in one launch of one workgroup,
the policy in LDS and the moments in registers) and scored by `amx_bcfit_eval`.
`plan_bc_batches` draws the mini-batch indices exactly as the reference's loop draws them; they
do not depend on the training, so they are drawn up front and numpy's global generator ends in
the state the reference leaves it in.

Same restrictions as the device policy and NPG kernels (npg.py:11-13): the (32, 32) tanh MLP,
identity input / output transformations, mini-batches of 64.
"""
from __future__ import annotations

import time as timer

import numpy as np
import torch

from . import _native as N
from .optstate import pack_state, policy_layout, read_state, write_state

BATCH = 64
HIDDEN = (32, 32)
LOSS_TYPES = {"MSE": N.AMX_BC_MSE, "MLE": N.AMX_BC_MLE}


def plan_bc_batches(num_samples: int, epochs: int, batch_size: int = BATCH) -> np.ndarray:
    """The index batches of BC.fit's loop (behavior_cloning.py:121-124): for every epoch,
    int(num_samples / batch_size) draws of np.random.choice(num_samples, size=batch_size) from
    numpy's global generator, in the reference's order -> int32 [epochs][steps][batch_size]."""
    steps = int(num_samples / batch_size)
    out = np.empty((epochs, steps, batch_size), dtype=np.int32)
    for ep in range(epochs):
        for mb in range(steps):
            out[ep, mb] = np.random.choice(num_samples, size=batch_size)
    return out


def _as_f32(x, device) -> torch.Tensor:
    """Host array or tensor -> contiguous fp32 on the device (torch.from_numpy(x).float(), once
    for the whole set)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.detach().to(torch.float32).to(device).contiguous()


class DeviceBC:
    """theta and torch.optim.Adam's state for the policy's S -> 32 -> 32 -> A tanh MLP, on the
    device.  `theta`: the reference's flat parameters (MLP.get_param_values' order; host array
    or device tensor; zeros when None)."""

    def __init__(self, ctx, theta=None, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, loss_type="MSE"):
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be 'MSE' or 'MLE', not {loss_type!r}")
        self.ctx = ctx
        self.S, self.A = ctx.S, ctx.A
        self.loss_type = loss_type
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), \
            float(weight_decay)
        self.layout = policy_layout(self.S, self.A, HIDDEN)
        self.P = self.layout.size
        assert self.P == ctx.lib.amx_npg_param_count(self.S, self.A)
        if ctx.lib.amx_bcfit_work(self.S, self.A) < 0:
            raise NotImplementedError(ctx.lib.amx_last_error().decode())
        self.theta = torch.zeros(self.P, dtype=torch.float32, device=ctx.device)
        if theta is not None:
            self.set_theta(theta)
        self._adam = None
        self._work = None
        self.step_losses = np.zeros(0, dtype=np.float32)  # the last fit's fp32 loss of every step

    def set_theta(self, theta) -> None:
        t = theta.detach() if isinstance(theta, torch.Tensor) else torch.from_numpy(np.asarray(theta))
        if t.numel() != self.P:
            raise ValueError(f"theta holds {t.numel()} values, the policy has {self.P}")
        self.theta.copy_(t.reshape(-1).to(torch.float32))

    # ---- Adam state (DeviceMLPBaseline's surface) -----------------------------------------------

    def _trained(self) -> int:
        """Parameters the loss trains: log_std has no gradient under MSE."""
        return 7 if self.loss_type == "MLE" else 6

    def _adam_state(self):
        if self._adam is None:
            dev = self.ctx.device
            self._adam = (torch.zeros(self.P, dtype=torch.float32, device=dev),
                          torch.zeros(self.P, dtype=torch.float32, device=dev),
                          torch.zeros(1, dtype=torch.int64, device=dev))
        return self._adam

    def load_optimizer(self, optimizer) -> None:
        """Adam state of a torch.optim.Adam over the policy's trainable_params (W1, b1, W2, b2,
        W3, b3, log_std) -> the device moments and step count.  Parameters without state load as
        zeros.  The device keeps one step count, so the trained parameters must agree on it."""
        kind, _, states = read_state(optimizer, kinds=("adam",))
        m, v = pack_state(self.layout, kind, states)
        steps = {step for step, _, _ in states[:self._trained()]}
        if len(steps) != 1:
            raise NotImplementedError(f"the trained parameters are at different Adam steps {sorted(steps)}")
        dm, dv, dstep = self._adam_state()
        dm.copy_(m)
        dv.copy_(v)
        dstep.fill_(steps.pop())

    def adam_state(self):
        """(step, [exp_avg per parameter], [exp_avg_sq per parameter]) on the host, in torch's
        parameter order and shapes (log_std's entries stay as loaded under MSE)."""
        dm, dv, dstep = self._adam_state()
        return int(dstep.item()), self.layout.unpack(dm.cpu()), self.layout.unpack(dv.cpu())

    # ---- the fit ----------------------------------------------------------------------------------

    def _eval(self, obs, act, out) -> None:
        c = self.ctx
        if self._work is None:
            self._work = torch.zeros(int(c.lib.amx_bcfit_work(self.S, self.A)) // 8, dtype=torch.float64,
                                     device=c.device)
        N.check(c.lib.amx_bcfit_eval(c.h, obs.shape[0], obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                     self.theta.data_ptr(), LOSS_TYPES[self.loss_type], self._work.data_ptr(),
                                     out.data_ptr(), c.stream), "amx_bcfit_eval")

    def loss(self, obs, act) -> float:
        """The loss of theta over all rows (BC.loss(data, idx=range(num_samples)))."""
        dev = self.ctx.device
        res = torch.zeros(1, dtype=torch.float64, device=dev)
        self._eval(_as_f32(obs, dev), _as_f32(act, dev), res)
        return float(res.item())

    def fit(self, obs, act, epochs: int, batches=None, max_steps_per_launch: int = 2048):
        """BC.fit's loop over `obs` [N, S] / `act` [N, A] (device tensors or host arrays; uploaded
        once as fp32): loss_before, `epochs` epochs of int(N / 64) Adam steps, loss_after.
        `batches`: int [epochs][steps][64] row indices (default: plan_bc_batches from numpy's
        global generator).  The steps run in launches of at most `max_steps_per_launch`; the cut
        changes no bit.  Returns (loss_before, [total loss per epoch], loss_after): each total is
        the double-precision sum of the steps' fp32 losses in step order."""
        c, dev = self.ctx, self.ctx.device
        obs, act = _as_f32(obs, dev), _as_f32(act, dev)
        n = obs.shape[0]
        if obs.dim() != 2 or obs.shape[1] != self.S or tuple(act.shape) != (n, self.A):
            raise ValueError(f"observations {tuple(obs.shape)} / actions {tuple(act.shape)} do not match S, A")
        if n < 1:
            raise ValueError("fit needs at least one row")
        if max_steps_per_launch < 1:
            raise ValueError("max_steps_per_launch must be positive")
        steps = int(n / BATCH)
        if batches is None:
            batches = plan_bc_batches(n, epochs)
        idx = np.ascontiguousarray(np.asarray(batches).reshape(epochs, steps, BATCH), dtype=np.int32)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"batches must hold row indices in [0, {n})")
        total = epochs * steps
        res = torch.zeros(2, dtype=torch.float64, device=dev)
        self._eval(obs, act, res[0:])
        if total:
            m, v, step = self._adam_state()
            idx_d = torch.from_numpy(idx.reshape(total, BATCH)).to(dev)
            losses = torch.zeros(total, dtype=torch.float32, device=dev)
            b1, b2 = self.betas
            for k0 in range(0, total, max_steps_per_launch):
                k = min(max_steps_per_launch, total - k0)
                N.check(c.lib.amx_bcfit_steps(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                              idx_d[k0:].data_ptr(), k, self.theta.data_ptr(), m.data_ptr(),
                                              v.data_ptr(), step.data_ptr(), self.lr, b1, b2, self.eps,
                                              self.weight_decay, LOSS_TYPES[self.loss_type], losses[k0:].data_ptr(),
                                              c.stream), "amx_bcfit_steps")
            self.step_losses = losses.cpu().numpy()
        else:
            self.step_losses = np.zeros(0, dtype=np.float32)
        self._eval(obs, act, res[1:])
        before, after = res.tolist()  # the fit's one host sync
        per_epoch = self.step_losses.reshape(epochs, steps)
        totals = []
        for ep in range(epochs):
            tot = 0.0
            for l in per_epoch[ep]:
                tot += float(l)  # total_loss += loss.item()
            totals.append(tot)
        return before, totals, after


class DataLog:
    """The part of mjrl's DataLog that BC writes: log_kv appends to self.log[key]."""

    def __init__(self):
        self.log = {}
        self.max_len = 0

    def log_kv(self, key, value):
        self.log.setdefault(key, []).append(value)
        self.max_len = max(self.max_len, len(self.log[key]))


def check_adam(optimizer) -> None:
    """The optimizers the policy fits implement: torch.optim.Adam, one group, no amsgrad / maximize."""
    read_state(optimizer, kinds=("adam",))


def write_optimizer(optimizer, d) -> None:
    """The device Adam state of `d` (adam_state, _trained) -> optimizer.state (step, exp_avg,
    exp_avg_sq per trained parameter), so a later fit, here or on the host, resumes where this
    one stopped."""
    step, ms, vs = d.adam_state()
    if step:
        write_state(optimizer, "adam", step, ms[:d._trained()], vs[:d._trained()])


class BC:
    """mjrl's BC (behavior_cloning.py:14-145) with the fit on the device.  `policy`: an mjrl MLP
    or any object with its attribute layout (model.fc_layers, log_std, trainable_params,
    get_param_values, set_param_values, m, min_log_std).  `ctx`: the AmxContext to run on (one
    is made for the policy's sizes when None)."""

    def __init__(self, expert_paths, policy, epochs=5, batch_size=64, lr=1e-3, optimizer=None, loss_type="MSE",
                 save_logs=True, set_transforms=False, ctx=None, **kwargs):
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be 'MSE' or 'MLE', not {loss_type!r}")
        if set_transforms:
            raise NotImplementedError("set_transforms=True: the device policy assumes identity transformations")
        tr = getattr(policy.model, "transformations", None)
        if tr and any(x is not None for x in tr.values()):
            raise NotImplementedError("the policy's model has input / output transformations: the device policy "
                                      "assumes identity transformations")
        layers = list(policy.model.fc_layers)
        hidden = tuple(l.weight.shape[0] for l in layers[:-1])
        if hidden != HIDDEN:
            raise NotImplementedError(f"the device fit supports hidden sizes {HIDDEN}, not {hidden}")
        if batch_size != BATCH:
            raise NotImplementedError(f"the device fit supports batch_size {BATCH}, not {batch_size}")
        if optimizer is not None:
            check_adam(optimizer)
        self.policy = policy
        self.expert_paths = expert_paths
        self.epochs = epochs
        self.mb_size = batch_size
        self.loss_type = loss_type
        self.save_logs = save_logs
        self.ctx = ctx
        self.device_bc = None
        self.optimizer = torch.optim.Adam(self.policy.trainable_params, lr=lr) if optimizer is None else optimizer
        self.logger = DataLog()

    def _device_bc(self) -> DeviceBC:
        """The engine object, built on first use with the optimizer's current hyper-parameters."""
        S, A = self.policy.model.fc_layers[0].weight.shape[1], self.policy.model.fc_layers[-1].weight.shape[0]
        if self.ctx is None:
            from .engine import AmxContext
            self.ctx = AmxContext(S, A)
        if (self.ctx.S, self.ctx.A) != (S, A):
            raise ValueError("the policy's sizes do not match the context's S, A")
        g = self.optimizer.param_groups[0]
        hyper = dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
        if self.device_bc is None:
            self.device_bc = DeviceBC(self.ctx, loss_type=self.loss_type, **hyper)
        d = self.device_bc
        d.lr, d.betas, d.eps, d.weight_decay = float(hyper["lr"]), tuple(map(float, hyper["betas"])), \
            float(hyper["eps"]), float(hyper["weight_decay"])
        return d

    def fit(self, data, suppress_fit_tqdm=False, **kwargs):
        assert all(k in data.keys() for k in ["observations", "expert_actions"])
        ts = timer.time()
        num_samples = data["observations"].shape[0]
        d = self._device_bc()
        d.set_theta(self.policy.get_param_values())
        d.load_optimizer(self.optimizer)
        print(f"Num samples: {num_samples}")
        obs, act = _as_f32(data["observations"], d.ctx.device), _as_f32(data["expert_actions"], d.ctx.device)
        before, totals, after = d.fit(obs, act, self.epochs)
        for ep, total_loss in enumerate(totals):
            print(f"Total loss for epoch {ep}: {total_loss}")
        write_optimizer(self.optimizer, d)
        params_after_opt = d.theta.cpu().numpy()
        self.policy.set_param_values(params_after_opt, set_new=True, set_old=True)
        clamped = self.policy.get_param_values()
        if self.save_logs and not np.array_equal(clamped, params_after_opt):
            # the reference scores loss_after with the written-back policy (log_std clamped at
            # min_log_std); the device keeps the unclamped theta
            after = DeviceBC(d.ctx, clamped, loss_type=self.loss_type).loss(obs, act)
        if self.save_logs:
            self.logger.log_kv("loss_before", np.float32(before))
            self.logger.log_kv("epoch", self.epochs)
            self.logger.log_kv("loss_after", np.float32(after))
            self.logger.log_kv("time", (timer.time() - ts))

    def train(self, **kwargs):
        observations = np.concatenate([path["observations"] for path in self.expert_paths])
        expert_actions = np.concatenate([path["actions"] for path in self.expert_paths])
        data = dict(observations=observations, expert_actions=expert_actions)
        self.fit(data, **kwargs)
