"""Device NPG policy update: the learner step that consumes the rollout
(mjrl NPG.train_from_paths, mjrl/mjrl/algos/npg_cg.py:113-199), next to the rollout engine.

The per-sample work (policy forward, Jacobian-vector products, back-propagation and the
reduction of per-sample gradients) is the HIP kernel `amx_npg_pass` (csrc/amx_npg.hip); the
10-iteration conjugate gradient (mjrl/mjrl/utils/cg_solve.py) is fp64 vector algebra on the
device between passes.  Parameters live in the reference's flat order (MLP.trainable_params:
W1, b1, W2, b2, W3, b3, log_std — gaussian_mlp.py:44-62), so `get_param_values` /
`set_param_values` exchange the same vectors as the reference policy.

Same semantics as the reference without input normalization (FCNetwork's default
in_shift/in_scale: (x - 0) / (1 + 1e-8) == x in float32); input normalization raises.  A
subsampled Fisher (hvp_sample_frac < 1, npg_cg.py:90-94) runs the Fisher-vector pass over an index
vector (amx_npg_pass_idx), one vector per CG iteration drawn from numpy's global generator as the
reference draws them; the BC term of NPG.CPI_surrogate (npg_cg.py:79-84) is one more VPG pass over
the expert rows with every advantage equal to reg_coeff, and a log-likelihood pass (amx_npg_ll) for
the surrogate's values.

With the rollout sharded over ranks the update runs data-parallel (`allreduce=`):
each rank passes its own rows, the passes divide by the global row count (amx_npg_pass_dp), and the
whitening records, the gradient, every CG iteration's Fisher-vector product and the evaluation sums
cross the ranks as one small fp64 all-reduce each.

`NPG` is the drop-in (the reference's constructor, `train_from_paths(paths, infos)`, `logger`,
`running_score`), built like ppo.PPO: `class NPG(amx.NPG, BatchREINFORCE): pass`.
"""
from __future__ import annotations

import math
import time as timer

import numpy as np
import torch

from . import _native as N
from .engine import AmxContext
from .gae import whiten_grid

NPG_VPG, NPG_FVP, NPG_EVAL = 0, 1, 2


def pack_policy(layers, log_std) -> np.ndarray:
    """[(W1, b1), (W2, b2), (W3, b3)], log_std -> the reference's flat fp32 parameter vector."""
    parts = []
    for W, b in layers:
        parts += [np.asarray(torch.as_tensor(W).detach().cpu().float()).ravel(),
                  np.asarray(torch.as_tensor(b).detach().cpu().float()).ravel()]
    parts.append(np.asarray(torch.as_tensor(log_std).detach().cpu().float()).ravel())
    return np.concatenate(parts).astype(np.float32)


def unpack_policy(flat, S: int, A: int, hidden=(32, 32)):
    """Inverse of pack_policy: ([(W, b)] * 3, log_std) as CPU float32 tensors."""
    flat = np.asarray(flat, dtype=np.float32)
    sizes = (S,) + tuple(hidden) + (A,)
    layers, i = [], 0
    for k in range(len(sizes) - 1):
        o, n = sizes[k + 1], sizes[k]
        W = torch.from_numpy(flat[i:i + o * n].reshape(o, n).copy())
        i += o * n
        b = torch.from_numpy(flat[i:i + o].copy())
        i += o
        layers.append((W, b))
    return layers, torch.from_numpy(flat[i:i + A].copy())


def paths_to_arrays(paths):
    """mjrl path dicts -> the concatenated observations, actions and advantages, and base_stats
    [mean, std, min, max] of the path returns (DeviceNPG's and DevicePPO's train_from_paths)."""
    obs, act, adv = (np.concatenate([p[k] for p in paths]) for k in ("observations", "actions", "advantages"))
    returns = [float(np.sum(p["rewards"])) for p in paths]
    return obs, act, adv, [float(np.mean(returns)), float(np.std(returns)), float(np.min(returns)),
                           float(np.max(returns))]


def engine_rows(engine, advantages: torch.Tensor, S: int, A: int):
    """The rollout engine's recorded transitions obs[:T], acts[:T] and the GAE advantages [T, B] as
    [T * B] rows, without a host round trip (DeviceNPG's and DevicePPO's train_from_engine)."""
    T, B = engine.t, engine.B
    return engine.obs[:T].reshape(T * B, S), engine.acts[:T].reshape(T * B, A), advantages.reshape(T * B)


class DeviceNPG:
    """NPG (npg_cg.py:26-199) for the mjrl Gaussian MLP policy, on the device.

    `policy_layers`/`log_std`: the current policy (nn.Linear layout).  `policy` (optional): a
    DevicePolicy to refresh after every update (the rollout's sampler)."""

    def __init__(self, ctx: AmxContext, policy_layers, log_std, normalized_step_size=0.01, const_learn_rate=None,
                 FIM_invert_args=None, hvp_sample_frac=1.0, kl_dist=None, min_log_std=-3.0,
                 input_normalization=None, policy=None, residual_tol=1e-10):
        if input_normalization:
            raise NotImplementedError("running input normalization is not implemented")
        if len(policy_layers) != 3 or any(W.shape[0] != 32 for W, _ in policy_layers[:2]):
            raise NotImplementedError("the device NPG kernel supports the (32, 32) tanh MLP (MILO's actor)")
        self.ctx = ctx
        self.S, self.A = ctx.S, ctx.A
        if policy_layers[0][0].shape[1] != self.S or policy_layers[2][0].shape[0] != self.A:
            raise ValueError("policy shapes do not match the context's S, A")
        FIM_invert_args = FIM_invert_args or {"iters": 10, "damping": 1e-4}
        self.cg_iters = int(FIM_invert_args["iters"])
        self.cg_fold = True  # the CG vector step folded into the next Fisher-vector pass
        self.damping = float(FIM_invert_args["damping"])
        self.alpha = const_learn_rate
        self.n_step_size = normalized_step_size if kl_dist is None else 2.0 * kl_dist
        self.min_log_std = float(min_log_std)
        self.residual_tol = residual_tol
        self.policy = policy
        self.hvp_subsample = hvp_sample_frac  # < 0.99: the Fisher on int(frac * N) rows drawn per CG iteration
        self.bc = None            # (expert_obs, expert_act, reg_coeff): the BC term of CPI_surrogate
        self.dist_info = False    # return old_dist_info / new_dist_info / lr
        self.eval_before = False  # compute surr_before (always with a BC term)
        self.hvp_products = 0     # Fisher-vector products the last subsampled solve took
        self.P = int(ctx.lib.amx_npg_param_count(self.S, self.A))
        self.theta = torch.from_numpy(pack_policy(policy_layers, log_std)).to(ctx.device)
        assert self.theta.numel() == self.P
        self._bufs = {}

    # ---- parameters (reference flat order) ----------------------------------------------
    def get_param_values(self) -> np.ndarray:
        return self.theta.cpu().numpy().copy()

    def set_param_values(self, new_params) -> None:
        """MLP.set_param_values (gaussian_mlp.py:71-94): float32, log_std clamped at min_log_std.
        A device tensor stays on the device (no host round trip)."""
        if isinstance(new_params, torch.Tensor):
            t = new_params.detach().to(self.ctx.device, torch.float32).clone()
        else:
            t = torch.as_tensor(np.asarray(new_params), dtype=torch.float32).to(self.ctx.device).clone()
        t[-self.A:] = torch.clamp(t[-self.A:], min=self.min_log_std)
        self.theta = t.contiguous()
        if self.policy is not None:
            self.policy.sync_from(*self._layers_view())

    def _layers_view(self):
        """([(W, b)] * 3, log_std) as device views of theta (reference flat order)."""
        sizes = (self.S, 32, 32, self.A)
        layers, i = [], 0
        for k in range(3):
            o, n = sizes[k + 1], sizes[k]
            W = self.theta[i:i + o * n].view(o, n)
            i += o * n
            layers.append((W, self.theta[i:i + o]))
            i += o
        return layers, self.theta[i:i + self.A]

    # ---- passes --------------------------------------------------------------------------
    def _rows_per_block(self, n: int) -> int:
        # one block per CU (the pass kernel holds ~140 KB of LDS): one wave of blocks
        return max(32, int(math.ceil(n / 256 / 32)) * 32)

    def _reduce(self, part, blocks: int, width: int, out, gate=None):
        """out[width] = the column sums of the [blocks][width] partials in block order
        (amx_npg_reduce_gated; behind `gate`, a stopped solve's state, it leaves `out` alone)."""
        c = self.ctx
        N.check(c.lib.amx_npg_reduce_gated(c.h, part.data_ptr(), blocks, width, out.data_ptr(), N.ptr(gate), c.stream),
                "amx_npg_reduce")
        return out

    def _pass(self, mode, obs, act, adv, vec, gate=None, hcache=None, reduce=True, out=None, part=None,
              n_total=None):
        """One pass (amx_npg_pass_ex) and its block-order reduction (into `out` when given);
        reduce=False returns the [blocks][width] partials instead (the CG folds their reduction
        into its step).  `part`: the rows of a larger partials buffer to write (no reduction).
        `n_total`: the divisor of a data-parallel update (amx_npg_pass_dp: the rows of every rank)."""
        c = self.ctx
        n = obs.shape[0]
        rpb = self._rows_per_block(n)
        nb = (n + rpb - 1) // rpb
        width = 2 if mode == NPG_EVAL else self.P
        key = (nb, width)
        if part is not None:
            assert part.shape == (nb, width) and part.is_contiguous()
            reduce = False
        else:
            part = self._bufs.get(key)
        if part is None:
            part = self._bufs[key] = torch.empty(nb, width, dtype=torch.float64, device=c.device)
        od = N.AMX_IN_F64 if obs.dtype == torch.float64 else N.AMX_IN_F32
        ad = N.AMX_IN_F64 if act.dtype == torch.float64 else N.AMX_IN_F32
        args = (c.h, mode, n, obs.data_ptr(), od, obs.stride(0), act.data_ptr(), ad, act.stride(0), N.ptr(adv),
                self.theta.data_ptr(), N.ptr(vec), rpb, part.data_ptr(), N.ptr(gate), N.ptr(hcache))
        if n_total is None:
            N.check(c.lib.amx_npg_pass_ex(*args, c.stream), "amx_npg_pass")
        else:
            N.check(c.lib.amx_npg_pass_dp(*args, int(n_total), c.stream), "amx_npg_pass_dp")
        if not reduce:
            return part
        if out is None:
            out = torch.empty(width, dtype=torch.float64, device=c.device)
        return self._reduce(part, nb, width, out, gate)

    def _inputs(self, observations, actions, advantages=None):
        dev = self.ctx.device
        obs = torch.as_tensor(observations).to(dev)
        act = torch.as_tensor(actions).to(dev)
        # the policy reads float32(obs) / float32(act) (gaussian_mlp.py:112-117): one cast here
        # serves every pass of the update and lets the pass kernel take 64-row chunks
        obs = obs.to(torch.float32).contiguous()
        act = act.to(torch.float32).contiguous()
        if obs.dim() != 2 or obs.shape[1] != self.S or act.shape != (obs.shape[0], self.A):
            raise ValueError(f"observations {tuple(obs.shape)} / actions {tuple(act.shape)} do not match S, A")
        adv = None
        if advantages is not None:
            adv = torch.as_tensor(advantages).to(dev, torch.float64).contiguous()
            if adv.numel() != obs.shape[0]:
                raise ValueError("advantages must have one entry per observation")
        return obs, act, adv

    def _pass_idx(self, obs, idx, vec, gate=None, hcache=None, count=None):
        """The Fisher-vector pass over the rows obs[idx] (amx_npg_pass_idx; idx: device int32 [M],
        0 <= idx < N): the [blocks][P] partials of the plain pass on the materialised rows."""
        c = self.ctx
        m = idx.numel()
        if obs.dtype != torch.float32 or idx.dtype != torch.int32 or not idx.is_contiguous() or m == 0:
            raise ValueError("the indexed pass takes fp32 observations and a non-empty contiguous int32 index vector")
        rpb = self._rows_per_block(m)
        nb = (m + rpb - 1) // rpb
        part = self._bufs.get((nb, self.P))
        if part is None:
            part = self._bufs[(nb, self.P)] = torch.empty(nb, self.P, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_npg_pass_idx(c.h, obs.shape[0], m, idx.data_ptr(), obs.data_ptr(), N.AMX_IN_F32,
                                       obs.stride(0), self.theta.data_ptr(), vec.data_ptr(), rpb, part.data_ptr(),
                                       N.ptr(gate), N.ptr(hcache), N.ptr(count), c.stream), "amx_npg_pass_idx")
        return part

    def _index_table(self, idx, n: int):
        """Host or device row indices -> a contiguous device int32 tensor, range-checked on the
        host when they come from there (the kernels trust 0 <= idx < N)."""
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            return idx.to(torch.int32).contiguous()
        a = np.ascontiguousarray(np.asarray(idx), dtype=np.int32)
        if a.size == 0 or a.min() < 0 or a.max() >= n:
            raise ValueError(f"row indices must be a non-empty set in [0, {n})")
        return torch.from_numpy(a).to(self.ctx.device)

    def log_likelihood(self, obs, act, theta=None, rows=False, out=None):
        """sum_r LL_r of the rows at `theta` (default: the current parameters) as a device fp64
        scalar in out[0] (amx_npg_ll's block partials, summed in block order); rows=True also
        returns every row's LL (fp32 [N]) and policy mean (fp32 [N][A])."""
        c = self.ctx
        n = obs.shape[0]
        theta = self.theta if theta is None else theta
        nb = int(c.lib.amx_npg_ll_blocks(c.h, n))
        part = torch.empty(nb, dtype=torch.float64, device=c.device)
        ll = torch.empty(n, dtype=torch.float32, device=c.device) if rows else None
        mean = torch.empty(n, self.A, dtype=torch.float32, device=c.device) if rows else None
        N.check(c.lib.amx_npg_ll(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                 theta.data_ptr(), part.data_ptr(), N.ptr(ll), N.ptr(mean), c.stream), "amx_npg_ll")
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=c.device)
        self._reduce(part, nb, 1, out)
        return (out, ll, mean) if rows else out

    def _vpg(self, obs, act, adv, hcache=None, bc=None, n_total=None) -> torch.Tensor:
        """The gradient of CPI_surrogate at new == old.  With a BC term: the rollout's VPG partials
        and those of the expert rows with every advantage equal to reg_coeff (the pass divides by
        its own N: reg_coeff * mean(LL)'s gradient) in one buffer, summed by one reduction, the
        rollout's blocks first.  `n_total`: _pass' (a data-parallel update takes no BC term)."""
        if bc is None:
            return self._pass(NPG_VPG, obs, act, adv, None, hcache=hcache, n_total=n_total)
        c = self.ctx
        eo, ea, reg = bc
        nb, nbe = (math.ceil(x.shape[0] / self._rows_per_block(x.shape[0])) for x in (obs, eo))
        part = torch.empty(nb + nbe, self.P, dtype=torch.float64, device=c.device)
        self._pass(NPG_VPG, obs, act, adv, None, hcache=hcache, part=part[:nb])
        eadv = torch.full((eo.shape[0],), float(reg), dtype=torch.float64, device=c.device)
        self._pass(NPG_VPG, eo, ea, eadv, None, part=part[nb:])
        return self._reduce(part, nb + nbe, self.P, torch.empty(self.P, dtype=torch.float64, device=c.device))

    def _bc_inputs(self, bc):
        if bc is None:
            return None
        eo, ea, reg = bc
        eo, ea, _ = self._inputs(eo, ea)
        return eo, ea, float(reg)

    def flat_vpg(self, observations, actions, advantages, bc=None) -> torch.Tensor:
        """BatchREINFORCE.flat_vpg (batch_reinforce.py:58-62) at new == old: fp64 [P]."""
        obs, act, adv = self._inputs(observations, actions, advantages)
        return self._vpg(obs, act, adv, bc=self._bc_inputs(bc))

    def _ls_curvature(self) -> torch.Tensor:
        """d^2 mean_kl / d log_std^2 at new == old (gaussian_mlp.py:144-155 with Dr's 1e-8):
        (8 s^2 - 4 s eps) / (2 s + eps)^2, s = exp(log_std)^2 -- one launch (amx_npg_curvature)."""
        c = self.ctx
        curv = torch.empty(self.A, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_npg_curvature(c.h, self.theta.data_ptr(), self.P, self.A, curv.data_ptr(), c.stream),
                "amx_npg_curvature")
        return curv

    def HVP(self, observations, actions, vector, regu_coef=None, idx=None) -> torch.Tensor:
        """NPG.HVP (npg_cg.py:87-106): Fisher (mean_kl Hessian) times `vector` + damping.  `idx`:
        the rows of the subsampled Fisher (the reference's rand_idx)."""
        obs, act, _ = self._inputs(observations, actions)
        if idx is not None:
            idx = self._index_table(idx, obs.shape[0]).reshape(-1)
        return self._hvp(obs, act, torch.as_tensor(vector).to(self.ctx.device), regu_coef, idx)

    def _hvp(self, obs, act, v, regu_coef=None, idx=None):
        regu = self.damping if regu_coef is None else regu_coef
        v32 = v.to(torch.float32).contiguous()   # the reference casts the vector to float32
        if idx is None:
            h = self._pass(NPG_FVP, obs, act, None, v32)
        else:
            part = self._pass_idx(obs, idx, v32)
            h = self._reduce(part, part.shape[0], self.P,
                             torch.empty(self.P, dtype=torch.float64, device=self.ctx.device))
        h[-self.A:] += self._ls_curvature() * v32[-self.A:].double()
        return h + regu * v.to(torch.float64)  # hvp_flat + regu_coef * vector (npg_cg.py:105: the fp64 vector)

    def _hcache(self, n: int) -> torch.Tensor:
        """The per-sample theta forward (H1 | H2, [n][64] fp32) the VPG pass writes and the CG's
        Fisher-vector passes read (amx_npg_pass_ex), grown on demand."""
        hc = self._bufs.get("hcache")
        if hc is None or hc.shape[0] < n:
            hc = self._bufs["hcache"] = torch.empty(n, 64, dtype=torch.float32, device=self.ctx.device)
        return hc

    def cg_solve(self, obs, act, b: torch.Tensor, hcache=None, idx=None, count=None, *, n_total=None,
                 allreduce=None) -> torch.Tensor:
        """mjrl/mjrl/utils/cg_solve.py:3-23 (starts from zeros; stops at rdotr < tol) with
        NPG.HVP as the operator.  Each iteration is one Fisher-vector pass and one column-sum
        launch (amx_npg_cg_reduce: z and the p.z parts per block); the vector step (x, r, p from
        fixed-order block parts) runs at the head of the NEXT iteration's pass (amx_npg_pass_cg,
        the same bits as the step's own launch) and once more, alone, after the last
        (amx_npg_cg_xrp).  `cg_fold = False` runs the round-5 form instead: the pass on p32, then
        amx_npg_cg_tail (the reduction and the step in two launches).  The early stop is the
        device-side `live` flag (a finished solve leaves x unchanged), so no host sync between
        iterations; after the stop the passes and reductions are empty launches.  `hcache`: the
        theta forward written by this update's VPG pass (train_from_arrays), so every product
        skips layers 1-2 at theta (bit-identical products).  `idx`: a device int32 [iters][M]
        table, iteration i's product on the rows obs[idx[i]] (NPG.HVP's subsampled Fisher, one
        draw per product); `count` (device fp64 [1], zeroed by the caller) then counts the
        products taken, i.e. the draws the reference's loop makes before its break.

        `allreduce` (with `n_total`, the rows of every rank): one rank's solve of a data-parallel
        update.  The passes divide by n_total (amx_npg_pass_dp, amx_npg_pass_cg_dp); the rank's
        column sums leave as one [P] message (amx_npg_reduce_gated), are summed over the ranks, and
        amx_npg_cg_reduce runs on the summed message as a one-block partials buffer: z, p.z and the
        vector step are formed from the same bits on every rank.  The host cannot see the early
        stop, so it always runs cg_iters collectives; a stopped solve (the same stop on every
        rank) leaves the message alone: the collective then re-sums finite values nobody reads."""
        c = self.ctx
        P = self.P
        dev = c.device
        fold = self.cg_fold
        if allreduce is not None and (idx is not None or not fold):
            raise NotImplementedError("the data-parallel solve is the folded one on all of the rank's rows")
        b = b.to(torch.float64).contiguous()
        if idx is not None:
            if idx.dim() != 2 or idx.shape[0] < self.cg_iters or idx.dtype != torch.int32 or not idx.is_contiguous():
                raise ValueError("idx must be a contiguous int32 [cg_iters][M] device table")
            if obs.dtype != torch.float32:
                raise ValueError("the subsampled Fisher takes fp32 observations")
        x, r, p, r2, p2 = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(5))
        p32, p32b = (torch.empty(P, dtype=torch.float32, device=dev) for _ in range(2))
        state, state2 = (torch.empty(2, dtype=torch.float64, device=dev) for _ in range(2))
        curv = torch.empty(self.A, dtype=torch.float64, device=dev)  # the log_std curvature, same launch
        msg = None if allreduce is None else torch.zeros(P, dtype=torch.float64, device=dev)
        N.check(c.lib.amx_npg_cg_init_ls(c.h, P, self.A, self.theta.data_ptr(), curv.data_ptr(), b.data_ptr(),
                                         x.data_ptr(), r.data_ptr(), p.data_ptr(), p32.data_ptr(), state.data_ptr(),
                                         c.stream), "amx_npg_cg_init_ls")
        work = self._bufs.get("cg_work")
        if work is None:
            work = self._bufs["cg_work"] = torch.empty(int(c.lib.amx_npg_cg_tail_work(P)), dtype=torch.float64,
                                                       device=dev)
        hc = hcache if obs.dtype == torch.float32 else None
        n = obs.shape[0]
        rpb = self._rows_per_block(n if idx is None else idx.shape[1])
        od = N.AMX_IN_F64 if obs.dtype == torch.float64 else N.AMX_IN_F32
        for it in range(self.cg_iters):
            if it == 0 or not fold:  # the product with p32 alone
                if idx is None:
                    part = self._pass(NPG_FVP, obs, act, None, p32, gate=state, hcache=hc, reduce=False,
                                      n_total=n_total)
                else:
                    part = self._pass_idx(obs, idx[it], p32, gate=state, hcache=hc, count=count)
            else:
                # the previous iteration's vector step, then the product with its p'; r, p, p32
                # and the state alternate buffers (every block reads all of them)
                args = (obs.data_ptr(), od, obs.stride(0), self.theta.data_ptr(), rpb, part.data_ptr(), N.ptr(hc),
                        self.residual_tol, x.data_ptr(), r.data_ptr(), r2.data_ptr(), p.data_ptr(), p2.data_ptr(),
                        p32b.data_ptr(), state.data_ptr(), state2.data_ptr(), work.data_ptr())
                if idx is not None:
                    N.check(c.lib.amx_npg_pass_cg_idx(c.h, n, idx.shape[1], idx[it].data_ptr(), *args, N.ptr(count),
                                                      c.stream), "amx_npg_pass_cg_idx")
                elif n_total is None:
                    N.check(c.lib.amx_npg_pass_cg(c.h, n, *args, c.stream), "amx_npg_pass_cg")
                else:
                    N.check(c.lib.amx_npg_pass_cg_dp(c.h, n, *args, int(n_total), c.stream), "amx_npg_pass_cg_dp")
                r, r2, p, p2, p32, p32b, state, state2 = r2, r, p2, p, p32b, p32, state2, state
            if not fold:
                # the partials' column sums and the vector step (amx_npg_cg_tail: two launches); r
                # and the state alternate buffers from one iteration to the next
                N.check(c.lib.amx_npg_cg_tail(c.h, part.data_ptr(), part.shape[0], P, self.A, curv.data_ptr(),
                                              self.damping, self.residual_tol, x.data_ptr(), r.data_ptr(),
                                              r2.data_ptr(), p.data_ptr(), p32.data_ptr(), state.data_ptr(),
                                              state2.data_ptr(), work.data_ptr(), c.stream), "amx_npg_cg_tail")
                r, r2, state, state2 = r2, r, state2, state
                continue
            z, blocks = part, part.shape[0]
            if allreduce is not None:  # the rank's column sums, summed over the ranks: one block
                allreduce(self._reduce(part, blocks, P, msg, gate=state))
                z, blocks = msg, 1
            N.check(c.lib.amx_npg_cg_reduce(c.h, z.data_ptr(), blocks, P, self.A, curv.data_ptr(), self.damping,
                                            p.data_ptr(), p32.data_ptr(), state.data_ptr(), work.data_ptr(),
                                            c.stream), "amx_npg_cg_reduce")
        if fold and self.cg_iters > 0:
            N.check(c.lib.amx_npg_cg_xrp(c.h, P, self.residual_tol, x.data_ptr(), r.data_ptr(), r2.data_ptr(),
                                         p.data_ptr(), p32.data_ptr(), state.data_ptr(), state2.data_ptr(),
                                         work.data_ptr(), c.stream), "amx_npg_cg_xrp")
        return x

    def surrogate_kl(self, obs, act, adv_w, new_theta) -> tuple[float, float]:
        """(CPI_surrogate, kl_old_new) of new_theta against the current parameters."""
        tot = self._pass(NPG_EVAL, obs, act, adv_w, new_theta.to(torch.float32).contiguous())
        n = obs.shape[0]
        return float(tot[0]) / n, float(tot[1]) / n

    # ---- the update ------------------------------------------------------------------------
    def draw_hvp_rows(self, n: int):
        """The reference's draws for one solve (NPG.HVP, npg_cg.py:90-92): cg_iters vectors of
        int(frac * n) rows from numpy's global generator, in its order.  Returns the int32
        [iters][M] table and the generator's state after 0, 1, ... iters draws."""
        m = int(self.hvp_subsample * n)
        if m < 1:
            raise ValueError(f"hvp_sample_frac {self.hvp_subsample} leaves no row of {n}")
        states, rows = [np.random.get_state()], []
        for _ in range(self.cg_iters):
            rows.append(np.random.choice(n, size=m))
            states.append(np.random.get_state())
        return np.asarray(rows, dtype=np.int32).reshape(self.cg_iters, m), states

    def _whiten(self, adv, allreduce=None, rank: int = 0, world: int = 1) -> torch.Tensor:
        """(adv - mean) / (std + 1e-6), population std (batch_reinforce.py:284-285): amx_adv_whiten,
        or over the ranks' rows its two halves around the all-reduce of the [world][4] records."""
        c = self.ctx
        n = adv.numel()
        w = torch.empty_like(adv)
        if allreduce is None:
            return whiten_grid(c, 1, n, adv, n, eps=1e-6, out=w)[0]
        wmsg = torch.zeros(world, 4, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_adv_whiten_parts(c.h, 1, n, None, None, n, adv.data_ptr(), rank, world, wmsg.data_ptr(),
                                           c.stream), "amx_adv_whiten_parts")
        allreduce(wmsg)
        stats = torch.empty(2, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_adv_whiten_apply(c.h, 1, n, None, None, n, adv.data_ptr(), wmsg.data_ptr(), world, 1e-6,
                                           w.data_ptr(), stats.data_ptr(), c.stream), "amx_adv_whiten_apply")
        return w

    def _apply_step(self, vpg, npg, res) -> torch.Tensor:
        """gdot, the step size and the clamped new parameters in one launch (amx_npg_apply_step):
        res[:3] = [alpha, n_step_size, gdot]; returns the new theta, already float32 with the
        log_std clamp (set_param_values' form)."""
        c = self.ctx
        new = torch.empty(self.P, dtype=torch.float32, device=c.device)
        use_alpha = self.alpha is not None
        N.check(c.lib.amx_npg_apply_step(c.h, self.P, self.A, vpg.data_ptr(), npg.data_ptr(), self.theta.data_ptr(),
                                         int(use_alpha), float(self.alpha) if use_alpha else 0.0,
                                         float(self.n_step_size), self.min_log_std, new.data_ptr(), res.data_ptr(),
                                         c.stream), "amx_npg_apply_step")
        return new

    def train_from_arrays(self, observations, actions, advantages, whiten: bool = True, bc=None,
                          dist_info=None, idx=None, *, allreduce=None, rank: int = 0, world: int = 1) -> dict:
        """NPG.train_from_paths on concatenated arrays (npg_cg.py:113-199): whitening
        (batch_reinforce.py:284-285), VPG, CG, step size, update with the log_std clamp,
        surr_after and kl_dist.  Returns the reference's infos entries.

        `bc` (default self.bc): (expert_obs, expert_act, reg_coeff), the BC term of CPI_surrogate
        in the gradient, surr_before and surr_after.  `dist_info` (default self.dist_info): also
        old_dist_info / new_dist_info ([LL, mean, log_std]) and lr of the new parameters against
        the old, where the reference's last CPI_surrogate call takes them.  `idx`: the
        [cg_iters][M] rows of the subsampled Fisher; by default, with hvp_sample_frac < 0.99, they
        are drawn as the reference draws them and numpy's generator is left after as many draws
        as the solve took products.  Any of these, or `eval_before`, also computes surr_before and
        returns hvp_products; with none the update is the plain one (surr_before 0.0): the same
        launches in the same order, less theirs.

        `allreduce` (with `rank`, `world`; taken from torch.distributed's group when one is
        initialised): the rows are this rank's share of a data-parallel update over `world` ranks,
        the update is the union's; `allreduce(t)` sums a device tensor in place over the ranks, as
        RolloutEngine.relabel's.  None: the single-process update.  The collectives of one update,
        in this order on every rank (each on the context's stream order):
          1. the row counts, int64 [world] (slot `rank` = the local n; the one extra host sync);
          2. the whitening records, fp64 [world][4] (only with `whiten`);
          3. the VPG, fp64 [P];
          4. cg_iters messages, fp64 [P] (see cg_solve);
          5. the EVAL sums, fp64 [2].
        Every pass divides by the global count; vpg_grad, npg_grad, alpha, delta, the new theta,
        surr_after and kl_dist are global and, given a collective that leaves the same bits on
        every rank, identical on all of them; `advantages` are the rank's own rows whitened with
        the global statistics.  A rank without rows makes every rank raise the same ValueError
        after the count exchange; a BC term, a subsampled Fisher, dist_info or eval_before raise
        NotImplementedError before any collective (numpy's draw order has no multi-rank meaning)."""
        bc = self.bc if bc is None else bc
        dist_info = self.dist_info if dist_info is None else dist_info
        sub = idx is not None or (self.hvp_subsample is not None and self.hvp_subsample < 0.99)
        ext = bc is not None or dist_info or sub or self.eval_before
        dp = allreduce is not None
        if dp:
            from . import dist as D
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                rank, world = D.rank_world()
            rank, world = int(rank), int(world)
            if world < 1 or not 0 <= rank < world:
                raise ValueError(f"rank {rank} is not in a world of {world}")
            unsupported = [name for name, on in (("a BC term", bc is not None), ("dist_info", bool(dist_info)),
                                                 ("a subsampled Fisher (hvp_sample_frac < 0.99 or idx)", sub),
                                                 ("eval_before", self.eval_before),
                                                 ("cg_fold = False", not self.cg_fold)) if on]
            if unsupported:
                raise NotImplementedError("the data-parallel NPG update does not support " + ", ".join(unsupported))
        obs, act, adv = self._inputs(observations, actions, advantages)
        c, dev = self.ctx, self.ctx.device
        n = obs.shape[0]
        n_total = None  # the passes' divisor when it is not their own n
        if dp:
            counts = torch.zeros(world, dtype=torch.int64, device=dev)
            counts[rank] = n
            allreduce(counts)
            counts_h = [int(v) for v in counts.tolist()]
            empty = [r for r, v in enumerate(counts_h) if v <= 0]
            if empty:  # decided from the exchanged counts: the same error on every rank, no collective left open
                raise ValueError(f"rank {empty[0]} of {world} holds no rows (row counts {counts_h}): every rank of a "
                                 "data-parallel NPG update needs at least one")
            n_total = sum(counts_h)
        bc = self._bc_inputs(bc)
        states = None
        if sub and self.cg_iters > 0:
            if idx is None:
                idx, states = self.draw_hvp_rows(n)
            idx = self._index_table(idx, n)
            if idx.dim() != 2 or idx.shape[0] < self.cg_iters:
                raise ValueError(f"idx must hold {self.cg_iters} index vectors")
        else:
            idx = None
        if whiten:
            adv = self._whiten(adv, allreduce, rank, world)
        # [alpha, n_step_size, gdot | surr_after, kl], then only with `ext`, zeroed: [surr_before,
        # kl_before | products | sum LL(expert) at the old, at the new parameters]: the kernels write
        # the parts of one buffer, read back in one copy (no concatenation kernel)
        res = torch.zeros(10, dtype=torch.float64, device=dev) if ext else \
            torch.empty(5, dtype=torch.float64, device=dev)
        old = self.theta
        hc = self._hcache(n)
        vpg = self._vpg(obs, act, adv, hcache=hc, bc=bc, n_total=n_total)
        if dp:
            allreduce(vpg)
        count = None
        if ext:
            count = res[7:8]
            self._pass(NPG_EVAL, obs, act, adv, old, out=res[5:7])  # new == old: LR == 1 on every row
            if bc is not None:
                self.log_likelihood(bc[0], bc[1], old, out=res[8:9])
        npg = self.cg_solve(obs, act, vpg, hcache=hc, idx=idx, count=count, n_total=n_total, allreduce=allreduce)
        new = self._apply_step(vpg, npg, res)
        ev = res[3:5]
        self._pass(NPG_EVAL, obs, act, adv, new, out=ev, n_total=n_total)  # plain sums: the host divides
        if dp:
            allreduce(ev)
        if bc is not None:
            self.log_likelihood(bc[0], bc[1], new, out=res[9:10])
        out = {}
        if dist_info:
            _, ll_o, mean_o = self.log_likelihood(obs, act, old, rows=True)
            _, ll_n, mean_n = self.log_likelihood(obs, act, new, rows=True)
            out = {"old_dist_info": [ll_o, mean_o, old[-self.A:].clone()],
                   "new_dist_info": [ll_n, mean_n, new[-self.A:].clone()], "lr": torch.exp(ll_n - ll_o)}
        self.theta = new
        if self.policy is not None:
            self.policy.sync_from(*self._layers_view())
        # the update's one host sync (after the counts' when data-parallel): the reference's infos
        # are python floats
        vals = res.tolist()
        alpha_h, delta_h, _, surr_h, kl_h = vals[:5]
        rows = n if n_total is None else n_total
        out.update({"vpg_grad": vpg, "npg_grad": npg, "alpha": alpha_h, "delta": delta_h, "surr_before": 0.0,
                    "surr_after": surr_h / rows, "kl_dist": kl_h / rows, "advantages": adv})
        if ext:
            sb_h, _, count_h, lle_o, lle_n = vals[5:]
            self.hvp_products = int(count_h) if idx is not None else 0
            if states is not None:  # the reference's loop stops drawing at its break (cg_solve.py:19-20)
                np.random.set_state(states[self.hvp_products])
            reg, ne = (bc[2], bc[0].shape[0]) if bc is not None else (0.0, 1)
            out.update({"surr_before": sb_h / n + reg * lle_o / ne, "surr_after": surr_h / n + reg * lle_n / ne,
                        "hvp_products": self.hvp_products})
        if dp:
            out["n_total"] = n_total
        return out

    def train_from_paths(self, paths, infos: dict | None = None, *, allreduce=None, rank: int = 0,
                         world: int = 1):
        """Reference surface: mjrl path dicts (observations, actions, advantages, rewards) ->
        base_stats [mean, std, min, max] of path returns; infos updated as the reference's.
        `allreduce`, `rank`, `world`: train_from_arrays' (the paths are this rank's; the returned
        statistics too)."""
        obs, act, adv, base_stats = paths_to_arrays(paths)
        out = self.train_from_arrays(obs, act, adv, allreduce=allreduce, rank=rank, world=world)
        if infos is not None:
            infos.update(out)
        return base_stats

    def train_from_engine(self, engine, advantages: torch.Tensor, *, allreduce=None, rank: int = 0,
                          world: int = 1) -> dict:
        """Update from the rollout engine's buffers without a host round trip: the recorded
        transitions obs[:T], acts[:T] ([T, B] rows) and GAE advantages [T, B].  `allreduce`, `rank`,
        `world`: train_from_arrays' (the engine's lanes are this rank's shard of the rollout)."""
        return self.train_from_arrays(*engine_rows(engine, advantages, self.S, self.A), allreduce=allreduce,
                                      rank=rank, world=world)


class NPG:
    """mjrl's NPG (npg_cg.py:25-199) with the update on the device: the reference's constructor,
    attributes, `train_from_paths(paths, infos)` and logger.  `policy`: an mjrl MLP or any object
    with its attribute layout (see ppo.PPO).  `ctx`: the AmxContext to run on (one is made for the
    policy's sizes when None).  train_step and the rollout statistics come from the reference's
    BatchREINFORCE: `class NPG(amx.NPG, BatchREINFORCE): pass`.  `allreduce` (keyword-only): the
    in-place SUM over the ranks of a sharded rollout (dist.allreduce_sum); the update is then the
    data-parallel one over every rank's paths (DeviceNPG.train_from_arrays), the advantages whitened on the
    device with the ranks' joint statistics, without a BC term, a subsampled Fisher or the dist-info
    entries of `infos`."""

    def __init__(self, env, policy, baseline, normalized_step_size=0.01, const_learn_rate=None,
                 FIM_invert_args={'iters': 10, 'damping': 1e-4}, hvp_sample_frac=1.0, seed=123, save_logs=False,
                 kl_dist=None, input_normalization=None,
                 bc_args={'flag': False, 'expert_paths': None, 'reg_coeff': None}, ctx=None, *, allreduce=None,
                 **kwargs):
        from .bc import HIDDEN, DataLog
        tr = getattr(policy.model, "transformations", None)
        if tr and any(x is not None for x in tr.values()):
            raise NotImplementedError("the policy's model has input / output transformations: the device policy "
                                      "assumes identity transformations")
        hidden = tuple(l.weight.shape[0] for l in list(policy.model.fc_layers)[:-1])
        if hidden != HIDDEN:
            raise NotImplementedError(f"the device update supports hidden sizes {HIDDEN}, not {hidden}")
        # the reference ignores values outside (0, 1] (npg_cg.py:61-63)
        if input_normalization is not None and 0 < input_normalization <= 1:
            raise NotImplementedError("running input normalization is not implemented")
        self.env = env
        self.policy = policy
        self.baseline = baseline
        self.alpha = const_learn_rate
        self.n_step_size = normalized_step_size if kl_dist is None else 2.0 * kl_dist
        self.seed = seed
        self.save_logs = save_logs
        self.FIM_invert_args = FIM_invert_args
        self.hvp_subsample = hvp_sample_frac
        self.running_score = None
        self.logger = DataLog()
        self.input_normalization = None
        self.bc_args = bc_args
        self.ctx = ctx
        # data-parallel: `paths` are this rank's, the update the union's (DeviceNPG.train_from_arrays; rank
        # and world from torch.distributed's group); running_score and the rollout statistics stay per rank
        self.allreduce = allreduce
        self.device_npg = None
        self._expert = None  # (host obs, host act, device obs, device act)

    def _device_npg(self) -> DeviceNPG:
        """The engine object, built on first use; this object's current settings."""
        pol = self.policy
        layers = [(l.weight, l.bias) for l in pol.model.fc_layers]
        S, A = layers[0][0].shape[1], layers[-1][0].shape[0]
        if self.ctx is None:
            self.ctx = AmxContext(S, A)
        if (self.ctx.S, self.ctx.A) != (S, A):
            raise ValueError("the policy's sizes do not match the context's S, A")
        if self.device_npg is None:
            self.device_npg = DeviceNPG(self.ctx, layers, pol.log_std, min_log_std=float(pol.min_log_std))
        d = self.device_npg
        d.alpha, d.n_step_size, d.hvp_subsample = self.alpha, self.n_step_size, self.hvp_subsample
        d.cg_iters, d.damping = int(self.FIM_invert_args["iters"]), float(self.FIM_invert_args["damping"])
        d.dist_info = d.eval_before = self.allreduce is None  # (not part of the data-parallel update)
        return d

    def _bc(self, d: DeviceNPG):
        """The expert rows on the device: uploaded once, again only when the arrays change."""
        b = self.bc_args
        if not b or not b.get("flag"):
            return None
        eo, ea = np.asarray(b["expert_paths"]["observations"]), np.asarray(b["expert_paths"]["actions"])
        e = self._expert
        if e is None or not (np.array_equal(e[0], eo) and np.array_equal(e[1], ea)):
            do, da, _ = d._inputs(eo, ea)
            e = self._expert = (eo.copy(), ea.copy(), do, da)
        return e[2], e[3], float(b["reg_coeff"])

    def train_from_paths(self, paths, infos):
        pol = self.policy
        # BatchREINFORCE.process_paths (batch_reinforce.py:271-297)
        observations = np.concatenate([path["observations"] for path in paths])
        actions = np.concatenate([path["actions"] for path in paths])
        advantages = np.concatenate([path["advantages"] for path in paths])
        if self.allreduce is None:  # (data-parallel: whitened on the device with the ranks' joint statistics)
            advantages = (advantages - np.mean(advantages)) / (np.std(advantages) + 1e-6)
        path_returns = [sum(p["rewards"]) for p in paths]
        mean_return = np.mean(path_returns)
        base_stats = [mean_return, np.std(path_returns), np.amin(path_returns), np.amax(path_returns)]
        self.running_score = mean_return if self.running_score is None else \
            0.9 * self.running_score + 0.1 * mean_return
        infos['advantages'] = advantages
        if self.save_logs and hasattr(self, "log_rollout_statistics"):
            self.log_rollout_statistics(paths)

        # the device update differentiates at new == old, as the reference's write-back leaves them
        cur = pol.get_param_values()
        old = np.concatenate([np.asarray(p.data.reshape(-1)) for p in pol.old_params])
        if not np.array_equal(cur, old):
            raise ValueError("policy.old_params differ from policy.trainable_params: the NPG update starts from "
                             "new == old (set_param_values(..., set_new=True, set_old=True))")
        ts = timer.time()
        d = self._device_npg()
        d.theta = torch.from_numpy(np.asarray(cur, dtype=np.float32)).to(d.ctx.device)  # as the policy holds them
        dp = self.allreduce is not None
        out = d.train_from_arrays(observations, actions, advantages, whiten=dp, bc=self._bc(d),
                                  allreduce=self.allreduce)
        new_params = d.theta.cpu().numpy()
        pol.set_param_values(new_params, set_new=True, set_old=True)
        t_upd = timer.time() - ts
        if dp:  # this rank's rows, whitened over all ranks; no per-row dist-info entries
            infos['advantages'] = out["advantages"].cpu().numpy()

        f32 = np.float32
        surr_before, surr_after, kl_dist = f32(out["surr_before"]), f32(out["surr_after"]), f32(out["kl_dist"])
        if not dp:
            infos['old_dist_info'] = [t.cpu() for t in out["old_dist_info"]]
            infos['new_dist_info'] = [t.cpu() for t in out["new_dist_info"]]
            infos['lr'] = out["lr"].cpu()
        infos['surr_before'] = surr_before
        if self.alpha is None:  # (npg_cg.py:157-161)
            infos['vpg_grad'] = out["vpg_grad"].cpu().numpy().astype(f32)
            infos['npg_grad'] = out["npg_grad"].cpu().numpy().astype(f32)
        infos['surr_after'] = surr_after
        if self.save_logs:
            self.logger.log_kv('alpha', out["alpha"])
            self.logger.log_kv('delta', out["delta"])
            # one device update: the gradient and the solve are not timed apart
            self.logger.log_kv('time_vpg', 0.0)
            self.logger.log_kv('time_npg', t_upd)
            self.logger.log_kv('kl_dist', kl_dist)
            self.logger.log_kv('surr_improvement', surr_after - surr_before)
            self.logger.log_kv('running_score', self.running_score)
            infos['surr_improvement'] = surr_after - surr_before
            infos['running_score'] = self.running_score
            infos['kl_dist'] = kl_dist
            infos['alpha'] = out["alpha"]
        return base_stats
