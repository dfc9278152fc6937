"""Device-backed drop-ins for the reference cost objects.

* `RBFLinearCost` — milo/milo/linear_cost.py:6-152 (MILO RFF MMD cost + pessimism bonus)
* `MLPCost`       — milo/milo/linear_cost.py:154-301: the same cost over MLP features
* `GAILCost`      — milo/milo/gail_cost.py:44-279: the AMP discriminator's reward + bonus and
                    its training step (update_disc, compute_chi2_distance) on the device.

Initialisation reproduces the reference's torch-CPU RNG stream exactly (seed, bandwidth
draw, nn.Linear construction order), so the same seed yields the same W, b, bandwidth and
discriminator weights; every per-sample computation then runs in the HIP kernels with the
expert features resident in HBM.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from .engine import AmxContext, RffMap, round_up, split_bf16x3, split_f16x2
from .optstate import common_step, disc_layout, pack_state, read_state, write_state


def device_discrepancy(ensemble, states, actions) -> torch.Tensor:
    """get_action_discrepancy (dynamics.py:154-165) left on the GPU, for any ensemble the
    surfaces accept (this package's DynamicsEnsemble / DeviceEnsemble, or the reference's own
    object, converted once: ensemble.as_device_ensemble)."""
    from .ensemble import as_device_ensemble
    return as_device_ensemble(ensemble).get_action_discrepancy(states, actions)

# cost-input row of a transition (linear_cost.py:115-127, gail_cost.py:258-268); "amp" is
# the AMP observation of (s, s') (SceneImitateAMP::BuildAMPObs, via a ReferenceMotion)
INPUT_TYPES = ("ss", "sa", "sas", "s", "amp")


def input_width(input_type: str, S: int, A: int, motion=None) -> int:
    """Width of the cost-input row of `input_type` for state size S and action size A."""
    if input_type == "amp":
        if motion is None:
            raise ValueError("input_type 'amp' needs the ReferenceMotion (motion=...)")
        return motion.amp_obs_size
    return {"ss": 2 * S, "sa": S + A, "sas": 2 * S + A, "s": S}[input_type]


def cost_input(input_type: str, states, actions, next_states, motion=None) -> torch.Tensor:
    """float32 cost-input rows [n, width] of `input_type` (the reference's torch.cat branches)."""
    if input_type == "sa":
        return torch.cat([states.float(), actions.float()], dim=1)
    if input_type == "ss":
        assert next_states is not None
        return torch.cat([states.float(), next_states.float()], dim=1)
    if input_type == "sas":
        return torch.cat([states.float(), actions.float(), next_states.float()], dim=1)
    if input_type == "s":
        return states.float()
    if input_type == "amp":
        assert next_states is not None and motion is not None
        return motion.amp_obs_from_states(states.double().contiguous(), next_states.double().contiguous()).float()
    raise NotImplementedError("Input type not implemented")


def _check_input_type(input_type: str, motion) -> None:
    if input_type not in INPUT_TYPES:
        raise NotImplementedError("Input type not implemented")
    if input_type == "amp" and motion is None:
        raise ValueError("input_type 'amp' needs the ReferenceMotion (motion=...)")


def fit_bandwidth(data: torch.Tensor, bw_samples: int, quantile: float) -> float:
    """The median-heuristic bandwidth of both MMD costs (linear_cost.py:73-82, 224-230): two
    torch.randint draws from the global generator, then the quantile of the pair distances."""
    n = data.shape[0]
    i0 = torch.randint(low=0, high=n, size=(bw_samples,))
    i1 = torch.randint(low=0, high=n, size=(bw_samples,))
    norm = torch.norm(data[i0, :] - data[i1, :], dim=1)
    return torch.quantile(norm, q=quantile).item()


class RBFLinearCost:
    """MMD cost with random-Fourier-feature representations (linear_cost.py:6-152).

    Same constructor arguments and methods as the reference; tensors returned by the
    cost methods live on the engine's device.
    """

    def __init__(self, expert_data: torch.Tensor, feature_dim=1024, input_type="ss", cost_range=(-1.0, 0.0),
                 bw_quantile=0.1, bw_samples=100000, lambda_b=1.0, lr=0.0, seed=100, ctx: AmxContext | None = None,
                 device="cuda", gemm: str = "f16x3", motion=None):
        """`gemm` selects the feature GEMM: "f16x3" (scaled 2-limb fp16 split) or "bf16x6"
        (3-limb bf16 split), both fp32-level error, or "f32" (f32 MFMA); `motion` (a
        ReferenceMotion) is needed for input_type "amp" (expert
        rows = AMP observations); everything else follows the reference constructor."""
        _check_input_type(input_type, motion)
        torch.manual_seed(seed)          # linear_cost.py:34-35
        np.random.seed(seed)
        expert_cpu = expert_data.detach().float().cpu()
        input_dim = expert_cpu.size(1)
        self.input_type = input_type
        self.input_dim = input_dim
        self.motion = motion
        self.feature_dim = feature_dim
        self.cost_range = cost_range
        if cost_range is not None:
            self.c_min, self.c_max = float(cost_range[0]), float(cost_range[1])
        self.lambda_b = float(lambda_b)
        self.lr = lr
        self.quantile = bw_quantile
        self.bw_samples = bw_samples
        self.bw = self.fit_bandwidth(expert_cpu)                  # :50 (torch-CPU RNG order)
        rff = nn.Linear(input_dim, feature_dim)                   # :53
        rff.bias.data = (torch.rand_like(rff.bias.data) - 0.5) * 2.0 * np.pi          # :54
        rff.weight.data = torch.rand_like(rff.weight.data) / (self.bw + 1e-8)          # :55
        self.rff_weight, self.rff_bias = rff.weight.data, rff.bias.data
        if ctx is None:
            S = input_dim // 2 if input_type == "ss" else input_dim
            ctx = AmxContext(S, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=feature_dim, device=device)
        self._embed_expert(ctx, RffMap(ctx, self.rff_weight, self.rff_bias, gemm=gemm), expert_cpu)

    def _embed_expert(self, ctx: AmxContext, fmap, expert_cpu: torch.Tensor) -> None:
        """The constructor's device half (no RNG is drawn here): the feature map, the expert
        features and phi_e, the relabel's buffers."""
        lambda_b = self.lambda_b
        self.ctx = ctx
        self.map = fmap
        self.w = None
        # expert features resident in HBM (:61-62); phi_e from fp64 column sums
        phi, tot = self.map.embed(expert_cpu)
        self.expert_rep = phi
        self.n_expert = expert_cpu.shape[0]
        self.phi_e = (tot / self.n_expert).float()
        self._expert_out = torch.empty(1 + 1024, dtype=torch.float64, device=ctx.device)
        self._expert_mean = None  # fp32 [1]: get_expert_cost's result (amx_expert_cost mean_out)
        # set when the last relabel_device launch also computed the expert cost for the current w
        self._expert_fresh = False
        self._counter = torch.zeros(4, dtype=torch.int32, device=ctx.device)  # amx_mmd_relabel's arrivals
        # expert rows this rank scores (shard_expert: a contiguous block per rank, partial sums
        # all-reduced asynchronously -- the expert cost only feeds the bonus_mmd log)
        self._elo, self._ehi = 0, self.n_expert
        self._ear = None   # allreduce_async of the sharded partial sum (None: one rank, whole buffer)
        self._eh = None    # the pending all-reduce handle of the last sharded partial sum
        self._estate = "global"  # sharded sum in _expert_out[0]: "partial" (this rank's) or "global"
        self._escale = torch.tensor([1.0 - lambda_b], dtype=torch.float32, device=ctx.device)

    # linear_cost.py:73-82
    def fit_bandwidth(self, data: torch.Tensor) -> float:
        return fit_bandwidth(data, self.bw_samples, self.quantile)

    def get_rep(self, x: torch.Tensor) -> torch.Tensor:
        """linear_cost.py:64-71."""
        return self.map.embed(x)[0]

    def fit_w_device(self, phi_sum: torch.Tensor, count: float) -> torch.Tensor:
        """Closed-form witness from an (already all-reduced) fp64 feature sum; returns w.w as
        a 1-element device tensor (no host synchronisation)."""
        c = self.ctx
        self._alloc_w()
        self._expert_fresh = False
        N.check(c.lib.amx_mmd_fit(c.h, phi_sum.data_ptr(), float(count), self.phi_e.data_ptr(), self.feature_dim,
                                  self.w.data_ptr(), self._mmd.data_ptr(), c.stream), "amx_mmd_fit")
        return self._mmd

    def _alloc_w(self) -> None:
        if self.w is None:
            c = self.ctx
            self.w = torch.empty(self.feature_dim, dtype=torch.float32, device=c.device)
            self._mmd = torch.empty(1, dtype=torch.float32, device=c.device)

    def shard_expert(self, rank: int, world: int, allreduce_async) -> None:
        """Score only this rank's contiguous block of the resident expert rows in the relabel
        and sum the ranks' fp64 partial sums with `allreduce_async(buf)` (returns a handle with
        .wait(), e.g. dist.all_reduce(async_op=True)), issued by expert_allreduce() off the
        rollout's critical path: get_expert_cost (linear_cost.py:105-109; bonus_mmd's expert
        term, batch_reinforce.py:169, a log value) waits for it when read.  SURVEY §8(e): phi_e
        replicated, the expert buffer's cost sharded, one scalar all-reduce for the log."""
        from .dist import shard
        if world > self.n_expert:
            raise ValueError(f"{self.n_expert} expert rows cannot be sharded over {world} ranks")
        self._elo, self._ehi = shard(self.n_expert, rank, world)
        self._ear = allreduce_async if world > 1 else None

    @property
    def expert_sharded(self) -> bool:
        return self._ear is not None

    def expert_allreduce(self):
        """Issue the all-reduce of the last relabel's partial expert sum (sharded mode, once per
        partial sum; no-op otherwise); returns the handle (the next relabel waits for it,
        GPU-side, before it overwrites the sum)."""
        if self._ear is None or not self._expert_fresh or self._estate != "partial":
            return None
        self._eh = self._ear(self._expert_out[:1])
        self._estate = "global"
        return self._eh

    def expert_allreduce_replayed(self):
        """expert_allreduce after a replayed graph whose relabel wrote a new partial sum (the
        graph's `after` hook: the captured launch does not pass through relabel_device)."""
        if self._ear is None or self.cost_range is None:
            return None
        self._expert_fresh, self._estate = True, "partial"
        return self.expert_allreduce()

    def wait_expert_allreduce(self) -> None:
        """Queue the wait (GPU-side) for the pending expert-sum all-reduce (graph replays call it
        before the graph whose relabel overwrites the sum; eager relabels call it themselves)."""
        if self._eh is not None and not torch.cuda.is_current_stream_capturing():
            self._eh.wait()
            self._eh = None

    def _expert_args(self):
        """(rows pointer, row count, mean_out) of the expert rows this rank scores."""
        ld = self.expert_rep.stride(0)
        ptr = self.expert_rep.data_ptr() + self._elo * ld * self.expert_rep.element_size()
        mean = None if self._ear is not None else self._expert_mean.data_ptr()
        return ptr, self._ehi - self._elo, mean

    def relabel_device(self, msg: torch.Tensor, phi, ldphi: int, disc, thr: float, reward, ipm, wb,
                       n: int) -> torch.Tensor:
        """The relabel tail in one launch (amx_mmd_relabel): w and w.w from the (all-reduced)
        [sum phi | count] message, the rewards of n rollout rows (raw device pointers), and,
        with a cost range, the expert cost for the new w (get_expert_cost then returns it
        without another pass).  Returns w.w (device, no host synchronisation)."""
        c = self.ctx
        self._alloc_w()
        expert = self.cost_range is not None
        if expert and self._expert_mean is None:
            self._expert_mean = torch.empty(1, dtype=torch.float32, device=c.device)
        self.wait_expert_allreduce()  # the previous partial sum's all-reduce reads the buffer this launch writes
        eptr, ne, emean = self._expert_args() if expert else (None, self.n_expert, None)
        N.check(c.lib.amx_mmd_relabel(c.h, msg.data_ptr(), 0.0, self.phi_e.data_ptr(), self.feature_dim,
                                      self.w.data_ptr(), self._mmd.data_ptr(), phi, ldphi, disc, float(thr),
                                      self.lambda_b, 1 if expert else 0, self.c_min if expert else 0.0,
                                      self.c_max if expert else 0.0, reward, ipm, wb, n,
                                      eptr, self.expert_rep.stride(0), ne, self._expert_out.data_ptr(),
                                      emean, self._counter.data_ptr(), c.stream), "amx_mmd_relabel")
        self._expert_fresh = expert
        if expert and self._ear is not None and not torch.cuda.is_current_stream_capturing():
            # (a captured launch: expert_allreduce_replayed after each replay).  The partial sum's
            # all-reduce is issued here, right behind the relabel, so every rank issues the same
            # collective sequence whether or not it later reads get_expert_cost (which only waits)
            self._estate = "partial"
            self.expert_allreduce()
        return self._mmd

    def fit_w(self, phi_sum: torch.Tensor, count: float) -> float:
        """fit_w_device + the reference's Python-float return (linear_cost.py:94)."""
        return float(self.fit_w_device(phi_sum, count).item())

    def fit_cost(self, data_pi: torch.Tensor) -> float:
        """linear_cost.py:84-94: w = mean phi(data_pi) - phi_e; returns w.w."""
        _, tot = self.map.embed(data_pi)
        return self.fit_w(tot, data_pi.shape[0])

    def _values(self, phi: torch.Tensor, disc: torch.Tensor, thr: float):
        c = self.ctx
        n = phi.shape[0]
        reward = torch.empty(n, dtype=torch.float32, device=c.device)
        ipm = torch.empty(n, dtype=torch.float32, device=c.device)
        wb = torch.empty(n, dtype=torch.float32, device=c.device)
        self.reward_launch(phi.data_ptr(), phi.stride(0), disc.data_ptr(), float(thr), reward.data_ptr(),
                           ipm.data_ptr(), wb.data_ptr(), n)
        return reward, ipm, wb

    def reward_launch(self, phi, ldphi: int, disc, thr: float, reward, ipm, wb, n: int) -> None:
        """amx_mmd_reward (cost_range given) or amx_mmd_reward_raw (cost_range None) on raw
        device pointers."""
        c = self.ctx
        if self.cost_range is not None:
            N.check(c.lib.amx_mmd_reward(c.h, phi, ldphi, self.w.data_ptr(), self.feature_dim, disc, thr,
                                         self.lambda_b, self.c_min, self.c_max, reward, ipm, wb, n, c.stream),
                    "amx_mmd_reward")
        else:
            N.check(c.lib.amx_mmd_reward_raw(c.h, phi, ldphi, self.w.data_ptr(), self.feature_dim, disc,
                                             self.lambda_b, reward, ipm, wb, n, c.stream), "amx_mmd_reward_raw")

    def get_costs(self, x: torch.Tensor) -> torch.Tensor:
        """linear_cost.py:96-103: clamp(phi(x).w, c_min, c_max) [n, 1] (unclamped when
        cost_range is None)."""
        phi = self.get_rep(x)
        n = phi.shape[0]
        zeros = torch.zeros(n, dtype=torch.float32, device=self.ctx.device)
        # with lambda = 0 the kernel's ipm output is exactly the clamped cost
        lam, self.lambda_b = self.lambda_b, 0.0
        try:
            _, ipm, _ = self._values(phi, zeros, 1.0)
        finally:
            self.lambda_b = lam
        return ipm.view(-1, 1)

    def get_expert_cost(self) -> torch.Tensor:
        """linear_cost.py:105-109 over the resident expert features."""
        if self.cost_range is None:   # the reference clamps with c_min/c_max, unset without a range
            raise AttributeError("'RBFLinearCost' object has no attribute 'c_min'")
        c = self.ctx
        if self._expert_mean is None:
            self._expert_mean = torch.empty(1, dtype=torch.float32, device=c.device)
        if self._ear is not None:  # sharded: this rank's partial sum, all-reduced
            if not self._expert_fresh:  # w changed since the last relabel: score this rank's block
                self.wait_expert_allreduce()
                eptr, ne, _ = self._expert_args()
                N.check(c.lib.amx_expert_cost(c.h, eptr, self.expert_rep.stride(0), self.w.data_ptr(),
                                              self.feature_dim, ne, self.c_min, self.c_max,
                                              self._expert_out.data_ptr(), None, float(self.lambda_b),
                                              c.stream), "amx_expert_cost")
                self._expert_fresh, self._estate = True, "partial"
            self.expert_allreduce()   # (no-op unless the sum is still this rank's partial)
            self.wait_expert_allreduce()
            # (1 - lambda) * float32(sum / n) as k_sum_small's mean_out (the fp32 product of torch)
            torch.mul((self._expert_out[:1] / self.n_expert).float(), self._escale, out=self._expert_mean)
            return self._expert_mean[0]
        if self._expert_fresh:  # computed for the current w by the relabel launch
            return self._expert_mean[0]
        N.check(c.lib.amx_expert_cost(c.h, self.expert_rep.data_ptr(), self.expert_rep.stride(0), self.w.data_ptr(),
                                      self.feature_dim, self.n_expert, self.c_min, self.c_max,
                                      self._expert_out.data_ptr(), self._expert_mean.data_ptr(),
                                      float(self.lambda_b), c.stream), "amx_expert_cost")
        # (1 - lambda) * mean in fp32 as the reference's torch expression; a 0-dim view of a
        # persistent buffer, overwritten by the next call
        return self._expert_mean[0]

    def get_bonus_costs(self, states, actions, ensemble, next_states=None):
        """linear_cost.py:111-152: cost [T, 1] and the info dict."""
        x = cost_input(self.input_type, states, actions, next_states, self.motion)
        phi = self.get_rep(x)
        disc = device_discrepancy(ensemble, states, actions)
        reward, ipm, wb = self._values(phi, disc, ensemble.threshold)
        cost = -reward
        rff_cost = self.get_costs(x)
        return cost.view(-1, 1), {"bonus": wb.view(-1, 1), "ipm": ipm.view(-1, 1), "v_targ": rff_cost,
                                  "cost": cost.view(-1, 1)}


def check_mlp_cost_config(hidden_dims, activation: str, feature_dim: int) -> None:
    """Refuse what MLPCost does not run on the device; raises before anything is built."""
    if activation != "relu":
        raise NotImplementedError(f"MLPCost on the device supports activation='relu' (both run.py branches); got "
                                  f"{activation!r} (the reference maps every other name to Tanh)")
    hidden_dims = list(hidden_dims)
    if len(hidden_dims) == 1 and hidden_dims[0] != feature_dim:
        raise NotImplementedError(
            f"hidden_dims={hidden_dims} with feature_dim={feature_dim}: with one hidden width the reference's net is "
            f"Linear(D, {hidden_dims[0]}) + Tanh alone (linear_cost.py:200-210 adds the feature layer only from the "
            f"second width on), so it emits features of width {hidden_dims[0]} yet scales them by "
            f"sqrt(2 / {feature_dim}); this quirk is not reproduced")
    if feature_dim <= 0 or feature_dim % 128:
        raise ValueError("feature_dim must be a multiple of 128 for the MFMA feature path")


def mlp_cost_net(input_dim: int, hidden_dims, feature_dim: int) -> nn.Sequential:
    """MLPCost's net on the host (linear_cost.py:199-212), ReLU between the layers: Linear(D, h0),
    [ReLU, Linear] per further hidden width, ReLU, Linear(., F), Tanh -- or Linear(D, F), Tanh
    without hidden widths.  The nn.Linear layers draw from torch's global generator in order, and
    the state_dict keys are the reference's ('0.weight', '2.weight', ...)."""
    hidden_dims = list(hidden_dims)
    dim = feature_dim if not hidden_dims else hidden_dims[0]
    layers = [nn.Linear(input_dim, dim)]
    if hidden_dims[1:]:
        for size in hidden_dims[1:]:
            layers += [nn.ReLU(), nn.Linear(dim, size)]
            dim = size
        layers += [nn.ReLU(), nn.Linear(dim, feature_dim)]
    layers.append(nn.Tanh())
    return nn.Sequential(*layers)


class MLPCost(RBFLinearCost):
    """MMD cost with MLP feature representations (linear_cost.py:154-301): phi(x) =
    cos(tanh(net(x))) sqrt(2/F) with a randomly initialised, untrained `net`.  After phi the
    algorithm is RBFLinearCost's, so everything but the feature map (MlpMap: the hidden layers on
    the f16x3 GEMM, the last Linear in amx_mlp_features_h3) is inherited: the resident expert
    features, phi_e and w from fp64 column sums, the clamp, the disagreement bonus, the expert
    cost and its sharding."""

    def __init__(self, expert_data: torch.Tensor, hidden_dims=[2048, 2048], activation="relu", feature_dim=1024,
                 input_type="ss", cost_range=[-1., 0.], bw_quantile=0.1, bw_samples=100000, lambda_b=1.0, lr=0.0,
                 seed=100, ctx: AmxContext | None = None, device="cuda", motion=None):
        """The reference's constructor arguments, then `ctx` / `device` / `motion` as RBFLinearCost.
        RNG order as the reference: the seeds, the nn.Linear layers in order, then the bandwidth
        draw (after the net here).  `net` stays on the host with the reference's keys, so
        save_checkpoint's cost_function.net.state_dict() (milo/utils.py:32-37) works as written."""
        _check_input_type(input_type, motion)
        check_mlp_cost_config(hidden_dims, activation, feature_dim)
        from .engine import MlpMap
        torch.manual_seed(seed)          # linear_cost.py:187-188
        np.random.seed(seed)
        expert_cpu = expert_data.detach().float().cpu()
        input_dim = expert_cpu.size(1)
        self.expert_data = expert_data
        self.input_type = input_type
        self.input_dim = input_dim
        self.motion = motion
        self.feature_dim = feature_dim
        self.hidden_dims = list(hidden_dims)
        self.cost_range = cost_range
        if cost_range is not None:
            self.c_min, self.c_max = float(cost_range[0]), float(cost_range[1])
        self.lambda_b = float(lambda_b)
        self.lr = lr
        self.activation = nn.ReLU()
        self.net = mlp_cost_net(input_dim, hidden_dims, feature_dim)      # :199-212
        self.quantile = bw_quantile
        self.bw_samples = bw_samples
        self.bw = self.fit_bandwidth(expert_cpu)                            # :217 (unused by the features)
        if ctx is None:
            S = input_dim // 2 if input_type == "ss" else input_dim
            ctx = AmxContext(S, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=feature_dim, device=device)
        linears = [m for m in self.net if isinstance(m, nn.Linear)]
        self._embed_expert(ctx, MlpMap(ctx, [(m.weight.data, m.bias.data) for m in linears]), expert_cpu)

    def get_expert_cost(self) -> torch.Tensor:
        """linear_cost.py:255-259 over the resident expert features."""
        if self.cost_range is None:   # the reference indexes cost_range, None without a range
            raise TypeError("'NoneType' object is not subscriptable")
        return super().get_expert_cost()


def plan_disc_batch(n_rb: int, n_expert: int, bs: int, sample_rb: bool):
    """The index draws of one GAILCost.update_disc (gail_cost.py:169-176) from numpy's global
    generator, in the reference's order: with sample_rb (mb_ss=None) the replay buffer's
    np.random.randint(0, n_rb, bs) first (datasets.py:101), then the expert's
    np.random.randint(0, n_expert, bs) (gail_cost.py:95).  Returns (agent rows in the buffer's
    logical order or None, expert rows)."""
    idx_m = np.random.randint(0, n_rb, bs) if sample_rb else None
    return idx_m, np.random.randint(0, n_expert, bs)


class _Disc(nn.Module):
    """Host mirror of the discriminator with the reference's state_dict keys (net.0, net.2, net.4)."""

    def __init__(self, layers):
        super().__init__()
        mods = []
        for i, lin in enumerate(layers):
            mods += ([nn.ReLU(inplace=True)] if i else []) + [lin]
        self.net = nn.Sequential(*mods)

    def forward(self, obs):
        return self.net(obs)


class GAILCost:
    """AMP/GAIL discriminator cost (gail_cost.py:44-279): rewards, bonus costs, and the
    discriminator's training (update_disc, compute_chi2_distance) on the device."""

    DISC_BATCH = 256      # rows update_disc samples when mb_ss is None (gail_cost.py:173)
    CHI2_CHUNK = 16384    # rows per inference pass of compute_chi2_distance

    def __init__(self, expert_data: torch.Tensor, agent_rb=None, feature_dim: int = 1, hidden_dims=(1024, 512),
                 input_type: str = "ss", scaling_coef: float = 0.5, reg_coef: float = 0.05, lambda_b: float = 0.5,
                 seed=100, grad_lambda=10.0, disc_loss_type="least_squares", disc_opt="sgd", disc_opt_args=None,
                 ctx: AmxContext | None = None, device="cuda", gemm: str = "f16x3", motion=None):
        """`motion` (a ReferenceMotion) is needed for input_type "amp" (discriminator on AMP
        observations); any disc_loss_type other than "least_squares" selects the
        log-likelihood cost, as in the reference's get_costs (gail_cost.py:246-251).  `gemm`:
        the discriminator layers' GEMM ("f16x3", "bf16x6" or "f32", as DeviceEnsemble)."""
        _check_input_type(input_type, motion)
        if feature_dim != 1:
            raise ValueError("Discriminator output must be 1-D")
        torch.manual_seed(seed)          # gail_cost.py:62-63
        np.random.seed(seed)
        self.expert_data = expert_data
        self.input_dim = expert_data.size(1)
        self.input_type = input_type
        self.motion = motion
        self.lambda_b = float(lambda_b)
        self.disc_loss_type = disc_loss_type
        self.loss_code = N.AMX_DISC_LEAST_SQUARES if disc_loss_type == "least_squares" else N.AMX_DISC_LOG_LIKELIHOOD
        sizes = [self.input_dim] + list(hidden_dims) + [1]
        layers = [nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]   # Discriminator :28-37
        for lin in layers:                                                             # disc_weight_init :11-16
            if lin.out_features == 1:
                nn.init.uniform_(lin.weight.data, a=-1.0, b=1.0)
            else:
                nn.init.xavier_uniform_(lin.weight.data)
        self.weights = [(l.weight.data.clone(), l.bias.data.clone()) for l in layers]
        # training (gail_cost.py:66-92): no RNG is drawn below
        self.online_rb = agent_rb
        self.n_expert_samples = expert_data.size(0)
        self.feature_dim = feature_dim
        self.scaling_coef, self.reg_coef, self.grad_lambda = float(scaling_coef), float(reg_coef), float(grad_lambda)
        opt_args = {"lr": 0.00001, "momentum": 0.9} if disc_opt_args is None else dict(disc_opt_args)
        self._opt_kind = "sgd" if disc_opt == "sgd" else "adam"
        self._opt_lr = float(opt_args["lr"])
        self._opt_p1 = float(opt_args["momentum"]) if self._opt_kind == "sgd" else 1e-8
        self._layers = layers
        self._disc = _Disc(layers)   # host mirror, synced from the device copy when that is newer
        self._disc_opt = None
        self._train = None           # device optimizer state and workspaces (first update_disc)
        self._steps = 0              # optimizer steps taken (the device's count)
        self._expert_dev = None
        if ctx is None:
            S = self.input_dim // 2 if input_type == "ss" else self.input_dim
            ctx = AmxContext(S, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=128, device=device)
        self.ctx = ctx
        if gemm not in ("f16x3", "bf16x6", "f32"):
            raise ValueError(f"gemm must be 'f16x3', 'bf16x6' or 'f32', got {gemm!r}")
        self.gemm = gemm
        self.load_weights(self.weights)
        self._dev_newer = False

    def load_weights(self, weights, optimizer=None) -> None:
        """Upload discriminator weights: a list of (W, b) pairs or a `disc.state_dict()`.
        `optimizer` (a `disc_opt.state_dict()`) also seeds the device optimizer state, to
        resume training from a checkpoint; without it the optimizer starts afresh."""
        if isinstance(weights, dict):
            n = len(weights) // 2
            weights = [(weights[f"net.{2 * i}.weight"], weights[f"net.{2 * i}.bias"]) for i in range(n)]
        widths = [int(W.shape[0]) for W, _ in weights[:-1]]
        self.Kin = round_up(self.input_dim, 32)
        layout = disc_layout(self.input_dim, self.Kin, widths, [round_up(h, 128) for h in widths])
        opt = None if optimizer is None else self._parse_optimizer(optimizer, layout)
        *hidden, w3, b3 = layout.views(layout.pack([t for Wb in weights for t in Wb]))
        dev = self.ctx.device
        self.layout = layout
        self.dev_layers = []
        k_pad = self.Kin
        for Wp, bp in zip(hidden[0::2], hidden[1::2]):
            out_p = Wp.shape[0]
            Wd = Wp.to(dev).contiguous()
            W3 = None
            if self.gemm == "bf16x6":
                W3 = split_bf16x3(self.ctx, Wd.unsqueeze(0))[0]
            elif self.gemm == "f16x3":
                W2, wexp = split_f16x2(self.ctx, Wd.unsqueeze(0))
                W3 = (W2[0], wexp[0])
            self.dev_layers.append((Wd, bp.to(dev).contiguous(), out_p, k_pad, W3))
            k_pad = out_p
        self.w3 = w3.reshape(-1).to(dev).contiguous()
        self.b3 = float(b3[0])
        self.h_last = k_pad
        self._ws = {}
        self._train, self._steps, self._disc_opt = None, 0, None
        self._dev_newer = True   # the host mirror follows the uploaded weights
        if opt is not None:
            self._opt_kind, self._opt_lr, self._opt_p1, self._steps, s1, s2 = opt
            t = self._train_state()
            t.step.fill_(self._steps)
            t.s1.copy_(s1)
            if s2 is not None:
                t.s2.copy_(s2)

    # ---- training: update_disc / compute_chi2_distance (gail_cost.py:94-228) ----------------

    _SUPPORTED = ("two hidden layers, trained by torch.optim.SGD(lr, momentum) without Nesterov, dampening or "
                  "weight decay, or by torch.optim.Adam(lr) with betas (0.9, 0.999), no weight decay, no amsgrad")

    def _check_trainable(self) -> None:
        if len(self._layers) != 3:
            raise NotImplementedError(f"update_disc on the device supports {self._SUPPORTED}; this discriminator "
                                      f"has {len(self._layers) - 1} hidden layer(s)")

    def _parse_optimizer(self, sd, layout):
        """(kind, lr, p1, steps, state1, state2) of a torch optimizer state_dict over the six tensors,
        the state in `layout`'s host vectors; refuses what amx_dfit_step does not cover, before
        anything is allocated."""
        if len(layout.live) != 6:
            raise NotImplementedError(f"update_disc on the device supports {self._SUPPORTED}; the weights given "
                                      f"have {len(layout.live) // 2 - 1} hidden layer(s)")
        kind, g, states = read_state(sd)
        if kind == "sgd":
            if g.get("nesterov") or g.get("weight_decay", 0) != 0:
                raise NotImplementedError(f"unsupported SGD options; supported: {self._SUPPORTED}")
            p1 = float(g["momentum"])
            steps = int(any(s1 is not None for _, s1, _ in states))   # SGD keeps no count
        else:
            if tuple(g["betas"]) != (0.9, 0.999) or g.get("weight_decay", 0) != 0:
                raise NotImplementedError(f"unsupported Adam options; supported: {self._SUPPORTED}")
            p1, steps = float(g["eps"]), common_step(states)
        return (kind, float(g["lr"]), p1, steps) + pack_state(layout, kind, states)

    def _train_state(self):
        """Device optimizer state beside the master weights (allocated once)."""
        if self._train is not None:
            return self._train
        self._check_trainable()
        from types import SimpleNamespace
        c, dev = self.ctx, self.ctx.device
        (_, _, H0p, Dp, _), (_, _, H1p, _, _) = self.dev_layers
        P = c.lib.amx_dfit_param_count(Dp, H0p, H1p)
        if P < 0:
            raise N.AmxNativeError("amx_dfit_param_count: " + c.lib.amx_last_error().decode())
        assert P == self.layout.size
        t = SimpleNamespace(P=P, work={}, idx={})
        t.s1 = torch.zeros(P, dtype=torch.float32, device=dev)
        t.s2 = torch.zeros(P, dtype=torch.float32, device=dev) if self._opt_kind == "adam" else None
        t.step = torch.zeros(1, dtype=torch.int64, device=dev)
        # one read-back per step: the 8 metrics (fp64) and, behind them, the master b2 [4] (fp32)
        t.rbuf = torch.zeros(10, dtype=torch.float64, device=dev)
        t.b2 = t.rbuf[8:].view(torch.float32)
        t.b2[0] = self.b3
        self._train = t
        return t

    def _expert_rows(self) -> torch.Tensor:
        if self._expert_dev is None:
            self._expert_dev = self.expert_data.detach().to(self.ctx.device, torch.float32).contiguous()
        return self._expert_dev

    def sample_from_expert_data(self, batch_size: int):
        """gail_cost.py:94-97."""
        idxs = np.random.randint(0, self.n_expert_samples, batch_size)
        return self.expert_data[idxs]

    def sample_from_online_buffer(self, batch_size: int):
        """gail_cost.py:99-102."""
        assert self.online_rb is not None, 'Cannot sample from nonexistent buffer.'
        return self.online_rb.sample(batch_size)

    def update_disc(self, mb_ss):
        """gail_cost.py:169-204 in one chain of launches (amx_dfit_step) on the fp32 master
        weights, then the refresh of the inference copies; one host synchronisation, the
        read-back of the metrics.  The index draws come from numpy's global generator in the
        reference's order (plan_disc_batch); with mb_ss=None the agent rows are read from the
        replay ring in place."""
        from .datasets import AgentReplayBuffer, ring_rows
        self._check_trainable()
        c, dev = self.ctx, self.ctx.device
        rb = None
        if mb_ss is None:
            assert self.online_rb is not None, 'need to sample from online buffer to get agent data!'
            rb = self.online_rb
            if not (isinstance(rb, AgentReplayBuffer) and rb.device == dev):
                mb_ss, rb = self.sample_from_online_buffer(self.DISC_BATCH), None
        if rb is not None:
            if len(rb) == 0:
                raise Exception('Not possible to sample from empty dataset.')
            if rb.ring.shape[1] != self.input_dim:
                raise ValueError(f"the replay buffer's rows have {rb.ring.shape[1]} entries, the discriminator's "
                                 f"input {self.input_dim}")
            bs = self.DISC_BATCH
            idx_m, idx_e = plan_disc_batch(len(rb), self.n_expert_samples, bs, True)
            idx_m = ring_rows(rb.head, rb.n, rb.max_size, idx_m)
            agent, n_agent = rb.ring, rb.max_size
        else:
            bs = mb_ss.size(0)
            _, idx_e = plan_disc_batch(0, self.n_expert_samples, bs, False)
            idx_m = None
            agent, n_agent = mb_ss.detach().to(dev, torch.float32).contiguous(), bs
            if agent.dim() != 2 or agent.shape[1] != self.input_dim:
                raise ValueError(f"mb_ss must be [n, {self.input_dim}], got {tuple(agent.shape)}")
        t = self._train_state()
        (W0, b0, H0p, Dp, _), (W1, b1, H1p, _, _) = self.dev_layers
        Bt = round_up(bs, 64)
        work = t.work.get(Bt)
        if work is None:
            nw = c.lib.amx_dfit_work_floats(Dp, H0p, H1p, Bt)
            if nw < 0:
                raise N.AmxNativeError("amx_dfit_work_floats: " + c.lib.amx_last_error().decode())
            work = t.work[Bt] = torch.empty(nw, dtype=torch.float32, device=dev)
            t.idx[Bt] = (torch.zeros(2, Bt, dtype=torch.int32).pin_memory(),
                         torch.zeros(2, Bt, dtype=torch.int32, device=dev))
        host_idx, dev_idx = t.idx[Bt]
        host_idx[0, :bs] = torch.from_numpy(idx_e.astype(np.int32))
        if idx_m is not None:
            host_idx[1, :bs] = torch.from_numpy(idx_m.astype(np.int32))
        dev_idx.copy_(host_idx, non_blocking=True)
        expert = self._expert_rows()
        adam = self._opt_kind == "adam"
        N.check(c.lib.amx_dfit_step(c.h, self.loss_code, N.AMX_DFIT_ADAM if adam else N.AMX_DFIT_SGD, self._opt_lr,
                                    self._opt_p1, self.scaling_coef, self.reg_coef, self.grad_lambda, bs, Bt,
                                    self.input_dim, Dp, H0p, H1p, dev_idx[0].data_ptr(),
                                    None if idx_m is None else dev_idx[1].data_ptr(), expert.data_ptr(),
                                    expert.stride(0), self.n_expert_samples, agent.data_ptr(), agent.stride(0),
                                    n_agent, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                    self.w3.data_ptr(), t.b2.data_ptr(), t.s1.data_ptr(), N.ptr(t.s2),
                                    t.step.data_ptr(), work.data_ptr(), t.rbuf.data_ptr(), c.stream), "amx_dfit_step")
        # the inference copies of the selected gemm follow the master weights (w3 is the master itself)
        for (Wd, _, _, _, W3) in self.dev_layers:
            if self.gemm == "f16x3":
                split_f16x2(c, Wd.unsqueeze(0), out=(W3[0].unsqueeze(0), W3[1].unsqueeze(0)))
            elif self.gemm == "bf16x6":
                split_bf16x3(c, Wd.unsqueeze(0), out=W3.unsqueeze(0))
        host = t.rbuf.cpu()   # the step's one host synchronisation
        self.b3 = float(host[8:].view(torch.float32)[0])
        self._steps += 1
        self._dev_newer = True
        m = host[:8].tolist()
        metrics = {'expert_disc_loss': m[0], 'model_based_disc_loss': m[1], 'gradient_penalty': m[2],
                   'regularizer_loss': m[3], 'total_disc_loss': m[4]}
        if self.loss_code == N.AMX_DISC_LEAST_SQUARES:
            metrics.update({'expert_acc': torch.tensor(m[5], dtype=torch.float32),
                            'mb_acc': torch.tensor(m[6], dtype=torch.float32)})
        return metrics

    def _sq_sum(self, table: torch.Tensor, idx: torch.Tensor | None, n: int, shift: float) -> torch.Tensor:
        """fp64 device sum of (D(row) + shift)^2 over rows idx (or the first n rows) of `table`,
        through the inference path in chunks."""
        acc = torch.zeros((), dtype=torch.float64, device=self.ctx.device)
        for lo in range(0, n, self.CHI2_CHUNK):
            hi = min(lo + self.CHI2_CHUNK, n)
            rows = table[lo:hi] if idx is None else table[idx[lo:hi]]
            xp, rows_p, k = self._pad(rows)
            logits = torch.empty(k, dtype=torch.float32, device=self.ctx.device)
            self.rewards_from_input(xp, rows_p, k, None, logits=logits)
            acc += ((logits.double() + shift) ** 2).sum()
        return acc

    @torch.no_grad()
    def compute_chi2_distance(self) -> float:
        """gail_cost.py:206-228: scaling_coef mean (D(expert) - 1)^2 + (1 - scaling_coef) mean
        (D(agent) + 1)^2 over the whole of the smaller set and as many sampled rows of the
        larger one (np.random.randint from the global generator, as the reference)."""
        from .datasets import AgentReplayBuffer, ring_rows
        assert self.online_rb is not None, 'Cannot compute divergence if there is no agent data.'
        rb, dev, ne = self.online_rb, self.ctx.device, self.n_expert_samples
        n = len(rb)
        if n == 0:
            raise Exception('Not possible to sample from empty dataset.')
        ring = isinstance(rb, AgentReplayBuffer) and rb.device == dev
        table = rb.ring if ring else torch.cat([rb.states, rb.next_states], dim=-1).to(dev, torch.float32)
        if n < ne:
            e_idx = torch.from_numpy(np.random.randint(0, ne, size=n)).to(dev)
            a_idx, cnt = None, n    # every held row once: the ring's physical rows [0, n)
        else:
            e_idx, cnt = None, ne
            a = np.random.randint(0, n, size=ne)
            a_idx = torch.from_numpy(ring_rows(rb.head, rb.n, rb.max_size, a) if ring else a).to(dev)
        se = self._sq_sum(self._expert_rows(), e_idx, cnt, -1.0)
        sa = self._sq_sum(table, a_idx, cnt, 1.0)
        return float(((self.scaling_coef * se + (1.0 - self.scaling_coef) * sa) / cnt).item())

    def _make_opt(self):
        if self._opt_kind == "sgd":
            return torch.optim.SGD(self._disc.parameters(), lr=self._opt_lr, momentum=self._opt_p1)
        return torch.optim.Adam(self._disc.parameters(), lr=self._opt_lr, eps=self._opt_p1)

    def sync_to_host(self) -> None:
        """Bring the host mirrors (`disc`, `disc_opt`) up to the device copy."""
        if self._disc_opt is None:
            self._disc_opt = self._make_opt()
        if not self._dev_newer:
            return
        padded = [t for Wd, bp, _, _, _ in self.dev_layers for t in (Wd, bp)] + [self.w3]
        flat = torch.cat([t.reshape(-1).cpu() for t in padded] + [torch.tensor([self.b3, 0.0, 0.0, 0.0])])
        with torch.no_grad():
            for p, live in zip(self._disc.parameters(), self.layout.unpack(flat)):
                p.copy_(live)
        self._disc_opt = self._make_opt()
        t = self._train
        if t is not None and self._steps > 0:
            write_state(self._disc_opt, self._opt_kind, self._steps, self.layout.unpack(t.s1.cpu()),
                        None if t.s2 is None else self.layout.unpack(t.s2.cpu()))
        self._dev_newer = False

    @property
    def disc(self):
        """The discriminator as a torch module with the reference's state_dict keys (net.0.weight
        .. net.4.bias), synced from the device copy when that is newer."""
        self.sync_to_host()
        return self._disc

    @property
    def disc_opt(self):
        """A torch.optim.SGD / Adam over `disc`'s parameters holding the device optimizer's
        state, so the reference's save_checkpoint (milo/utils.py:38-44) works as written."""
        self.sync_to_host()
        return self._disc_opt

    def _hidden(self, x_pad: torch.Tensor, rows: int, row_exp: torch.Tensor | None = None) -> torch.Tensor:
        """Hidden layers over `rows` padded input rows.  f16x3: `row_exp` [rows] int32 = the
        input rows' exponents (amx_step_rexp for the rollout's [s, s'] rows; None computes them);
        each layer's epilogue writes the exponents of its output rows for the next."""
        c = self.ctx
        ws = self._ws.get(rows)
        if ws is None:
            ws = [torch.empty(rows, L[2], dtype=torch.float32, device=c.device) for L in self.dev_layers]
            ws.append(torch.empty(len(self.dev_layers) + 1, rows, dtype=torch.int32, device=c.device))
            self._ws[rows] = ws
        h = x_pad
        if self.gemm == "f16x3":
            rexp = ws[-1]
            if row_exp is None:
                N.check(c.lib.amx_row_exponents(c.h, 1, rows, self.Kin, h.data_ptr(), h.stride(0), 0, rexp.data_ptr(),
                                                rows, 1, c.stream), "amx_row_exponents(disc)")
                src = rexp[0]
            else:
                src = row_exp
            rexp[1:].fill_(-100)
            for i, ((Wp, bp, out_p, k_pad, (W2, wexp)), o) in enumerate(zip(self.dev_layers, ws)):
                N.check(c.lib.amx_gemm_bias_act_h3(c.h, 1, rows, out_p, k_pad, h.data_ptr(), h.stride(0), 0,
                                                   W2.data_ptr(), 0, wexp.data_ptr(), 0, bp.data_ptr(), 0,
                                                   o.data_ptr(), out_p, 0, 0, N.AMX_ACT_RELU, src.data_ptr(), 0, 1,
                                                   rexp[i + 1].data_ptr(), 0, c.stream),
                        "amx_gemm_bias_act_h3(disc)")
                h, src = o, rexp[i + 1]
            return h
        for (Wp, bp, out_p, k_pad, W3), o in zip(self.dev_layers, ws):
            if W3 is not None:
                N.check(c.lib.amx_gemm_bias_act_x6(c.h, 1, rows, out_p, k_pad, h.data_ptr(), h.stride(0), 0,
                                                   W3.data_ptr(), 0, bp.data_ptr(), 0, o.data_ptr(), out_p, 0, 0,
                                                   N.AMX_ACT_RELU, c.stream), "amx_gemm_bias_act_x6(disc)")
            else:
                N.check(c.lib.amx_gemm_bias_act(c.h, 1, rows, out_p, k_pad, h.data_ptr(), h.stride(0), 0,
                                                Wp.data_ptr(), k_pad, 0, bp.data_ptr(), 0, o.data_ptr(), out_p, 0, 0,
                                                N.AMX_ACT_RELU, c.stream), "amx_gemm_bias_act(disc)")
            h = o
        return h

    def rewards_from_input(self, x_pad: torch.Tensor, rows: int, n: int, disc: torch.Tensor | None,
                           out: torch.Tensor | None = None, logits: torch.Tensor | None = None,
                           loss_code: int | None = None, row_exp: torch.Tensor | None = None) -> torch.Tensor:
        """Fused discriminator + reward on already padded input rows [rows, Kin]."""
        c = self.ctx
        h = self._hidden(x_pad, rows, row_exp)
        out = torch.empty(n, dtype=torch.float32, device=c.device) if out is None else out
        N.check(c.lib.amx_disc_reward(c.h, self.loss_code if loss_code is None else loss_code, h.data_ptr(),
                                      h.stride(0), self.h_last, self.w3.data_ptr(), self.b3,
                                      None if disc is None else disc.data_ptr(), self.lambda_b, out.data_ptr(),
                                      None if logits is None else logits.data_ptr(), n, c.stream), "amx_disc_reward")
        return out

    def _pad(self, x: torch.Tensor):
        n = x.shape[0]
        rows = round_up(max(n, 1), 128)
        xp = torch.zeros(rows, self.Kin, dtype=torch.float32, device=self.ctx.device)
        xp[:n, :self.input_dim] = x.to(self.ctx.device, torch.float32)
        return xp, rows, n

    def disc_logits(self, ss: torch.Tensor) -> torch.Tensor:
        xp, rows, n = self._pad(ss)
        logits = torch.empty(n, dtype=torch.float32, device=self.ctx.device)
        self.rewards_from_input(xp, rows, n, None, logits=logits)
        return logits.view(-1, 1)

    def get_ls_costs(self, ss: torch.Tensor) -> torch.Tensor:
        """gail_cost.py:231-236: -max(0, 1 - 0.25 (1 - D)^2)  [n, 1]."""
        xp, rows, n = self._pad(ss)
        return (-self.rewards_from_input(xp, rows, n, None, loss_code=N.AMX_DISC_LEAST_SQUARES)).view(-1, 1)

    def get_ll_costs(self, ss: torch.Tensor) -> torch.Tensor:
        """gail_cost.py:238-244: logsigmoid(D)  [n, 1]."""
        xp, rows, n = self._pad(ss)
        return (-self.rewards_from_input(xp, rows, n, None, loss_code=N.AMX_DISC_LOG_LIKELIHOOD)).view(-1, 1)

    def get_costs(self, ss: torch.Tensor) -> torch.Tensor:
        """gail_cost.py:246-251."""
        return self.get_ls_costs(ss) if self.loss_code == N.AMX_DISC_LEAST_SQUARES else self.get_ll_costs(ss)

    def get_bonus_costs(self, states, actions, ensemble, next_states=None):
        """gail_cost.py:254-279: cost = (1-lambda) * input cost - lambda * disagreement."""
        x = cost_input(self.input_type, states, actions, next_states, self.motion)
        xp, rows, n = self._pad(x)
        disc = device_discrepancy(ensemble, states, actions)
        reward = self.rewards_from_input(xp, rows, n, disc)
        input_cost = self.get_costs(x)
        lam = np.float32(self.lambda_b)
        ipm = np.float32(1 - self.lambda_b) * input_cost
        bonus = lam * disc.view(-1, 1)
        cost = (-reward).view(-1, 1)
        return cost, {"bonus": bonus, "ipm": ipm, "v_targ": input_cost, "cost": cost}
