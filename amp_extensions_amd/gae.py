"""Returns, the MLP value baseline and GAE on the device: the consumer of the sampler's
output in the reference's policy step (mjrl BatchREINFORCE.train_step,
mjrl/mjrl/algos/batch_reinforce.py:176-180, and process_paths :271-297).

Two layouts share the same kernels (include/amx_hip.h, "segment grid"):
  * the rollout engine's lane buffers ([T, B] rows, several trajectories per lane separated
    by done flags, trajectories that run past the buffer bootstrapped as non-terminated);
  * concatenated mjrl path dicts (`process_samples`), one lane per path — a drop-in for
    `process_samples.compute_returns` + `compute_advantages` (mjrl/mjrl/utils/process_samples.py).
The value MLP is the reference's MLPBaseline (mjrl/mjrl/baselines/mlp_baseline.py:10-108):
features [clip(obs,-10,10)/10, (t/1000)^1..4] -> Linear/ReLU ... -> Linear(., 1), run on the
MFMA GEMM with the hidden widths zero-padded to 128.  Fitting the baseline
(MLPBaseline.fit, mlp_baseline.py:61-97: mini-batch Adam through fit_data,
mjrl/mjrl/utils/optimize_model.py:7-36) runs on the device too (`fit`, `fit_grid`,
csrc/amx_vfit.hip) on the same feature rows; the weights and the Adam state live in device
memory, and `sync_to` writes both into an mjrl baseline where a checkpoint is taken.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from .engine import AmxContext, round_up
from .optstate import baseline_layout, common_step, pack_state, read_state, write_state


def init_mlp_baseline_params(inp_dim: int, hidden=(128, 128), seed: int | None = None):
    """Layers of MLPBaseline.model (mlp_baseline.py:20-27): nn.Linear(n+4 -> h1), ReLU, ...,
    nn.Linear(-> 1), default torch init drawn in layer order (after torch.manual_seed(seed)
    when a seed is given)."""
    if seed is not None:
        torch.manual_seed(seed)
    sizes = (inp_dim + 4,) + tuple(hidden) + (1,)
    layers = [nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]
    return [(l.weight.data.clone(), l.bias.data.clone()) for l in layers]


FIT_BATCH = 64    # mini-batch rows of the device fit
FIT_HIDDEN = 128  # widest hidden layer of the device fit


class DeviceMLPBaseline:
    """MLPBaseline.predict and MLPBaseline.fit on the device.  Workspace rows:
    [feat kf | h0 | h1 | ...] with kf = round_up(S+4, 32) and every hidden width padded to a
    multiple of 128.

    `learn_rate`, `reg_coef`, `batch_size`, `epochs` are MLPBaseline's constructor arguments
    (same defaults); `betas` / `eps` are torch.optim.Adam's.  The fit supports two hidden
    layers of width <= 128 and batch_size 64 (run.py's critic and MLPBaseline's default);
    `fit` raises NotImplementedError for anything else, prediction is not restricted.

    Single rank only: the fit runs over the rows this process holds.  With lanes sharded over
    ranks a global fit (every rank stepping the same weights over all ranks' rows) needs a
    design of its own and is not provided."""

    def __init__(self, ctx: AmxContext, layers, *, learn_rate: float = 1e-3, reg_coef: float = 0.0,
                 batch_size: int = 64, epochs: int = 1, betas=(0.9, 0.999), eps: float = 1e-8):
        self.ctx = ctx
        self.kf = round_up(ctx.S + 4, 32)
        self._ws = None
        self.learn_rate, self.reg_coef = float(learn_rate), float(reg_coef)
        self.batch_size, self.epochs = int(batch_size), int(epochs)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self._adam = None  # (m, v, step) device tensors, allocated by the first fit / optimizer load
        self._fit_work = None
        self.sync_from(layers)

    @classmethod
    def from_mjrl(cls, ctx: AmxContext, baseline):
        """Build from an mjrl `MLPBaseline`: its nn.Sequential of Linear/ReLU, batch_size and
        epochs, and its optimizer's hyper-parameters and state (step, exp_avg, exp_avg_sq;
        absent before the optimizer's first step)."""
        _, g, _ = read_state(baseline.optimizer, kinds=("adam",))
        self = cls(ctx, cls._layers_of(baseline), learn_rate=g["lr"], reg_coef=g["weight_decay"],
                   batch_size=baseline.batch_size, epochs=baseline.epochs, betas=g["betas"], eps=g["eps"])
        if self.fit_supported():  # a shape the fit refuses still predicts; it has no state to load
            self.load_optimizer(baseline.optimizer)
        return self

    @staticmethod
    def _layers_of(baseline):
        return [(m.weight.data, m.bias.data) for m in baseline.model if isinstance(m, nn.Linear)]

    def sync_from(self, layers, optimizer=None) -> None:
        """Upload (W [out, in], b) per layer; accepts the list or an mjrl MLPBaseline.  The
        Adam state is left alone unless `optimizer` (the torch.optim.Adam over the same
        parameters, in layer order) is given."""
        if hasattr(layers, "model"):
            layers = self._layers_of(layers)
        self._sync_weights(layers)
        if optimizer is not None:
            self.load_optimizer(optimizer)

    def _sync_weights(self, layers) -> None:
        c, dev = self.ctx, self.ctx.device
        if len(layers) < 2:
            raise ValueError("MLPBaseline needs at least one hidden layer")
        if layers[0][0].shape[1] != c.S + 4 or layers[-1][0].shape[0] != 1:
            raise ValueError(f"baseline layers must map {c.S + 4} features to 1 value")
        widths = [int(W.shape[0]) for W, _ in layers[:-1]]
        if self._adam is not None and widths != self.widths:
            self._adam = None  # another model: its moments do not carry over
        self.widths = widths
        self.Hp = [round_up(h, 128) for h in widths]
        self.layout = baseline_layout(c.S + 4, self.kf, widths, self.Hp)
        self.col = [0, self.kf]
        for hp in self.Hp:
            self.col.append(self.col[-1] + hp)
        self.ldv = self.col[-1]
        padded = self.layout.views(self.layout.pack([t for Wb in layers for t in Wb]))
        *hidden, w_head, self.b_head = [t.to(dev).contiguous() for t in padded]
        self.W, self.b, self.w_head = hidden[0::2], hidden[1::2], w_head.reshape(-1)

    def workspace(self, rows: int) -> torch.Tensor:
        rp = max(round_up(rows, 128), 128)
        if self._ws is None or self._ws.shape[0] < rp or self._ws.shape[1] != self.ldv:
            self._ws = torch.zeros(rp, self.ldv, dtype=torch.float32, device=self.ctx.device)
            self._v = torch.zeros(rp, dtype=torch.float32, device=self.ctx.device)
        return self._ws

    def predict_grid(self, rows: int, T: int, L: int, obs: torch.Tensor, ldo: int, end: torch.Tensor, stride: int,
                     lengths: torch.Tensor | None = None, t0: torch.Tensor | None = None,
                     base: torch.Tensor | None = None) -> torch.Tensor:
        """Baseline values of every grid row (rows = row-space size) -> f32 [rows_pad]."""
        self._features(rows, T, L, obs, ldo, end, stride, lengths, t0, base)
        return self._forward(rows)

    def _features(self, rows, T, L, obs, ldo, end, stride, lengths, t0, base) -> torch.Tensor:
        """MLPBaseline._features of every grid row into the workspace's first kf columns."""
        c = self.ctx
        ws = self.workspace(rows)
        N.check(c.lib.amx_value_features(c.h, T, L, _ptr(lengths), _ptr(t0), _ptr(base), stride, end.data_ptr(),
                                         obs.data_ptr(), ldo, ws.data_ptr(), self.ldv, c.stream), "amx_value_features")
        return ws

    def _forward(self, rows: int) -> torch.Tensor:
        """The model over the workspace's feature rows -> f32 [rows_pad]."""
        c = self.ctx
        ws = self.workspace(rows)
        rp = round_up(rows, 128)
        for i in range(len(self.Hp)):
            K = self.kf if i == 0 else self.Hp[i - 1]
            A = ws[:, self.col[i]:]
            N.check(c.lib.amx_gemm_bias_act(c.h, 1, rp, self.Hp[i], K, A.data_ptr(), self.ldv, 0, self.W[i].data_ptr(),
                                            K, 0, self.b[i].data_ptr(), 0, ws.data_ptr(), self.ldv, 0, self.col[i + 1],
                                            1, c.stream), "amx_gemm_bias_act")
        h = ws[:, self.col[-2]:]
        N.check(c.lib.amx_value_head(c.h, rp, h.data_ptr(), self.ldv, self.Hp[-1], self.w_head.data_ptr(),
                                     self.b_head.data_ptr(), self._v.data_ptr(), c.stream), "amx_value_head")
        return self._v[:rp]

    # ---- fit ---------------------------------------------------------------------------------

    def fit_supported(self) -> bool:
        return len(self.widths) == 2 and max(self.widths) <= FIT_HIDDEN and self.batch_size == FIT_BATCH

    def _check_fit_supported(self) -> None:
        if len(self.widths) != 2 or max(self.widths) > FIT_HIDDEN:
            raise NotImplementedError(f"the device fit supports two hidden layers of width <= {FIT_HIDDEN} "
                                      f"(MLPBaseline's default critic), not {tuple(self.widths)}")
        if self.batch_size != FIT_BATCH:
            raise NotImplementedError(f"the device fit supports batch_size {FIT_BATCH}, not {self.batch_size}")

    def _adam_state(self):
        if self._adam is None:
            P = self.layout.size
            assert P == self.ctx.lib.amx_vfit_param_count(self.kf, self.Hp[0], self.Hp[1])
            dev = self.ctx.device
            self._adam = (torch.zeros(P, dtype=torch.float32, device=dev),
                          torch.zeros(P, dtype=torch.float32, device=dev),
                          torch.zeros(1, dtype=torch.int64, device=dev))
        return self._adam

    def load_optimizer(self, optimizer) -> None:
        """Adam state of a torch.optim.Adam over the model's parameters (layer order: weight,
        bias per Linear) -> the device moments and step count.  Parameters without state (no
        step taken yet) load as zeros."""
        self._check_fit_supported()
        kind, _, states = read_state(optimizer, kinds=("adam",))
        step = common_step(states)
        m, v = pack_state(self.layout, kind, states)
        dm, dv, dstep = self._adam_state()
        dm.copy_(m)
        dv.copy_(v)
        dstep.fill_(step)

    def adam_state(self):
        """(step, [exp_avg per parameter], [exp_avg_sq per parameter]) on the host, in torch's
        parameter order and live (unpadded) shapes."""
        self._check_fit_supported()
        dm, dv, dstep = self._adam_state()
        return int(dstep.item()), self.layout.unpack(dm.cpu()), self.layout.unpack(dv.cpu())

    def layers(self):
        """[(W [out, in], b)] per layer on the host, live shapes (the inverse of sync_from)."""
        padded = [t for Wb in zip(self.W, self.b) for t in Wb] + [self.w_head, self.b_head]
        live = self.layout.unpack(torch.cat([t.reshape(-1) for t in padded]).cpu())
        return list(zip(live[0::2], live[1::2]))

    def sync_to(self, baseline) -> None:
        """Write the weights into `baseline.model` and the Adam state into `baseline.optimizer`
        (an mjrl MLPBaseline or anything with those two attributes), so that
        model.state_dict() / optimizer.state_dict() checkpoint what the device holds and a host
        fit continues where the device stopped."""
        lin = [m for m in baseline.model if isinstance(m, nn.Linear)]
        mine = self.layers()
        if [tuple(l.weight.shape) for l in lin] != [tuple(W.shape) for W, _ in mine]:
            raise ValueError("baseline.model's layers do not match the device baseline")
        with torch.no_grad():
            for l, (W, b) in zip(lin, mine):
                l.weight.copy_(W)
                l.bias.copy_(b)
        if self._adam is None:
            return
        step, ms, vs = self.adam_state()
        opt = baseline.optimizer
        if step == 0:
            for p in opt.param_groups[0]["params"]:
                opt.state.pop(p, None)
        else:
            write_state(opt, "adam", step, ms, vs)

    def fit_grid(self, rows: int, T: int, L: int, obs: torch.Tensor, ldo: int, end: torch.Tensor, stride: int,
                 returns: torch.Tensor, lengths: torch.Tensor | None = None, t0: torch.Tensor | None = None,
                 base: torch.Tensor | None = None, *, perms=None, return_errors: bool = False,
                 return_all_errors: bool = False):
        """MLPBaseline.fit over grid rows already on the device: `predict_grid`'s arguments plus
        `returns` (f32 or f64, one per row of the row space; cast to f32 on the device like the
        reference's returns.astype('float32')).  Every one of the `rows` rows must belong to the
        grid (engine buffers and concatenated paths do).  `epochs` epochs of int(rows / 64) - 1
        Adam steps each; epoch e batches rows through perms[e] (int array of `rows` indices) or,
        by default, np.random.permutation(rows) from numpy's global RNG, exactly as fit_data
        draws it.  Returns what MLPBaseline.fit returns."""
        self._check_fit_supported()
        if rows < 2 * self.batch_size:
            raise ValueError(f"fit needs at least {2 * self.batch_size} rows (int(rows / batch_size) - 1 steps), "
                             f"got {rows}")
        c, dev = self.ctx, self.ctx.device
        used = (rows // self.batch_size - 1) * self.batch_size  # rows the steps of an epoch read
        host_perms = []
        for ep in range(self.epochs):
            p = np.random.permutation(rows) if perms is None else np.asarray(perms[ep])
            if p.ndim != 1 or p.shape[0] < used or p.min() < 0 or p.max() >= rows:
                raise ValueError(f"perms[{ep}] must hold at least {used} row indices in [0, {rows})")
            host_perms.append(p.astype(np.int32))
        y = returns.reshape(-1)[:rows].to(torch.float32).contiguous()
        ws = self._features(rows, T, L, obs, ldo, end, stride, lengths, t0, base)

        def error():  # sum((returns - pred)^2) / (sum(returns^2) + 1e-8), mlp_baseline.py:82-83
            e = y - self._forward(rows)[:rows]
            return (torch.sum(e * e) / (torch.sum(y * y) + 1e-8)).cpu().numpy()[()]

        error_before = error() if return_errors else None
        m, v, step = self._adam_state()
        if self._fit_work is None:
            self._fit_work = torch.zeros(c.lib.amx_vfit_work(self.kf, self.Hp[0], self.Hp[1]) // 4,
                                         dtype=torch.float32, device=dev)
        losses = torch.zeros(max(self.epochs, 1), dtype=torch.float32, device=dev)
        for ep, p in enumerate(host_perms):
            perm_d = torch.from_numpy(p).to(dev)
            N.check(c.lib.amx_vfit_epoch(c.h, rows, ws.data_ptr(), self.ldv, y.data_ptr(), perm_d.data_ptr(), self.kf,
                                         self.Hp[0], self.Hp[1], self.W[0].data_ptr(), self.b[0].data_ptr(),
                                         self.W[1].data_ptr(), self.b[1].data_ptr(), self.w_head.data_ptr(),
                                         self.b_head.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(),
                                         self.learn_rate, self.betas[0], self.betas[1], self.eps, self.reg_coef,
                                         self._fit_work.data_ptr(), losses[ep:].data_ptr(), c.stream),
                    "amx_vfit_epoch")
        epoch_losses = [l.reshape(1) for l in losses[:self.epochs].cpu().numpy()]
        if return_errors:
            error_after = error()
            if return_all_errors:
                return error_before, error_after, epoch_losses
            return error_before, error_after
        return None

    def fit(self, paths, return_errors: bool = False, return_all_errors: bool = False, perms=None):
        """MLPBaseline.fit(paths, return_errors, return_all_errors) (mlp_baseline.py:61-97) on
        the device: `paths` are mjrl path dicts with "observations" and "returns"; returns
        (error_before, error_after[, epoch_losses]) like the reference when return_errors is
        set, else None.  The permutations come from numpy's global RNG as in fit_data (a caller
        who seeds numpy gets the reference's batches) unless `perms` injects one per epoch."""
        self._check_fit_supported()
        c, dev = self.ctx, self.ctx.device
        lens = np.array([len(p["observations"]) for p in paths], dtype=np.int64)
        n_rows = int(lens.sum())
        if n_rows < 2 * self.batch_size:
            raise ValueError(f"fit needs at least {2 * self.batch_size} rows (int(rows / batch_size) - 1 steps), "
                             f"got {n_rows}")
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        obs = torch.from_numpy(np.ascontiguousarray(np.concatenate([p["observations"] for p in paths]),
                                                    dtype=np.float64).reshape(n_rows, -1)).to(dev)
        ret = torch.from_numpy(np.concatenate([np.asarray(p["returns"]).reshape(-1) for p in paths])
                               .astype(np.float32)).to(dev)
        end = np.zeros(n_rows, dtype=np.uint8)
        end[(offs + lens - 1)[lens > 0]] = 1
        return self.fit_grid(n_rows, int(lens.max(initial=0)), len(paths), obs, c.S, torch.from_numpy(end).to(dev), 1,
                             ret, lengths=torch.from_numpy(lens.astype(np.int32)).to(dev),
                             base=torch.from_numpy(offs).to(dev), perms=perms, return_errors=return_errors,
                             return_all_errors=return_all_errors)


def _ptr(t):
    return None if t is None else t.data_ptr()


def gamma_lambda(gamma: float, gae_lambda) -> float:
    """compute_advantages' mode switch (process_samples.py:10): GAE for 0 <= lambda <= 1,
    the standard returns - baseline mode otherwise (encoded as a negative value)."""
    if gae_lambda is None or gae_lambda < 0.0 or gae_lambda > 1.0:
        return -1.0
    return float(gamma) * float(gae_lambda)


def gae_grid(ctx: AmxContext, T: int, L: int, end, rew, rstride: int, v, gamma: float, gae_lambda, stride: int,
             ret: torch.Tensor, adv: torch.Tensor, lengths=None, base=None, rbase=None) -> None:
    N.check(ctx.lib.amx_gae(ctx.h, T, L, _ptr(lengths), _ptr(base), stride, end.data_ptr(), rew.data_ptr(),
                            _ptr(rbase), rstride, v.data_ptr(), float(gamma), gamma_lambda(gamma, gae_lambda),
                            ret.data_ptr(), adv.data_ptr(), ctx.stream), "amx_gae")


def whiten_grid(ctx: AmxContext, T: int, L: int, adv: torch.Tensor, stride: int, eps: float = 1e-6,
                out: torch.Tensor | None = None, lengths=None, base=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(adv - mean) / (std + eps) over the grid rows (batch_reinforce.py:284-285); returns
    (out, stats[mean, std]) as device tensors."""
    out = adv if out is None else out
    stats = torch.empty(2, dtype=torch.float64, device=adv.device)
    N.check(ctx.lib.amx_adv_whiten(ctx.h, T, L, _ptr(lengths), _ptr(base), stride, adv.data_ptr(), float(eps),
                                   out.data_ptr(), stats.data_ptr(), ctx.stream), "amx_adv_whiten")
    return out, stats


def process_samples(paths, baseline: DeviceMLPBaseline, gamma: float, gae_lambda=None, normalize: bool = False):
    """mjrl `compute_returns(paths, gamma)` + `compute_advantages(paths, baseline, gamma,
    gae_lambda, normalize)` (process_samples.py:3-35) on the device for a list of path dicts.
    Writes path['returns'] (f64), path['baseline'] (f32) and path['advantages'] (f64) like
    the reference; returns the device tensors (concatenated path order)."""
    c = baseline.ctx
    dev = c.device
    lens = np.array([len(p["rewards"]) for p in paths], dtype=np.int64)
    n_rows = int(lens.sum())
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate([p["observations"] for p in paths]),
                                                dtype=np.float64)).to(dev)
    rew = torch.from_numpy(np.concatenate([np.asarray(p["rewards"], dtype=np.float32) for p in paths])).to(dev)
    end = np.zeros(n_rows, dtype=np.uint8)
    for p, o, l in zip(paths, offs, lens):
        if l:
            end[o + l - 1] = 1 if p.get("terminated", True) else 2
    end_d = torch.from_numpy(end).to(dev)
    lens_d = torch.from_numpy(lens.astype(np.int32)).to(dev)
    base_d = torch.from_numpy(offs).to(dev)
    T, L = int(lens.max(initial=0)), len(paths)
    v = baseline.predict_grid(n_rows, T, L, obs, c.S, end_d, 1, lengths=lens_d, base=base_d)
    ret = torch.empty(max(n_rows, 1), dtype=torch.float64, device=dev)
    adv = torch.empty_like(ret)
    gae_grid(c, T, L, end_d, rew, 1, v, gamma, gae_lambda, 1, ret, adv, lengths=lens_d, base=base_d, rbase=base_d)
    if normalize:  # process_samples.py:23-28 / 30-35 (eps 1e-8)
        whiten_grid(c, T, L, adv, 1, eps=1e-8, lengths=lens_d, base=base_d)
    ret_h, adv_h, v_h = ret.cpu().numpy(), adv.cpu().numpy(), v[:n_rows].cpu().numpy()
    for p, o, l in zip(paths, offs, lens):
        p["returns"] = ret_h[o:o + l].copy()
        p["baseline"] = v_h[o:o + l].copy()
        p["advantages"] = adv_h[o:o + l].copy()
    return ret[:n_rows], adv[:n_rows], v[:n_rows]
