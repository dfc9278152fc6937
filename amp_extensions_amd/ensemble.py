"""Drop-in `DynamicsEnsemble` (milo/milo/dynamics.py:19-165) over the device ensemble.

The constructor, `load_ensemble(path)`, `save_ensemble(path)`, `compute_threshold()`,
`threshold`, `get_action_discrepancy`, `compute_discrepancy` and `models[k].forward` take the
reference's arguments and keep its semantics, so run.py's own call sequence runs unchanged
(run.py:72-78, 105, 108):

    dynamic_ensemble = DynamicsEnsemble(state_size, action_size, offline_dataset, validate_dataset,
                                        num_models=..., batch_size=..., hidden_sizes=..., transform=...,
                                        dense_connect=..., optim_args=optim_args, base_seed=args.seed,
                                        device=torch.device('cpu'))
    dynamic_ensemble.load_ensemble(ensemble_path)
    dynamic_ensemble.compute_threshold()

`device` keeps the reference's meaning (where the caller's tensors live; run.py forces the CPU,
run.py:69): results come back there.  The arithmetic always runs on the GPU (`gpu=`, default
the current HIP device) through `DeviceEnsemble` -- there is no CPU path.  The members'
parameters and optimizers are also held on the host as plain nn.Linear containers with the
reference's state-dict keys (`fc_layers.{i}.weight/bias`), so the checkpoint format written by
the reference's `save_ensemble` (a list of {'model', 'optim'}, dynamics.py:110-116) loads and
saves unchanged (torch.load with weights_only=True: tensors and plain containers only).

Training (DynamicsEnsemble.train, dynamics.py:82-108, 236-378) runs on the device through
`train_on_device`, which takes `train`'s arguments and returns what it returns: all members
advance in lock step, each on the index batches the reference's DataLoaders would have drawn
for it (`plan_batches`).  `train()` itself keeps raising and names that method (a pinned
test requires the raise).  `DynamicsEnsemble` implements the dense-connect ReLU BasicMLP
(dynamics.py:394-433, the README command's `--dynamic_dense_connect`) and
`PlainDynamicsEnsemble` the plain one (`dense_connect=False`, run.py's default: layer i reads
layer i-1's output only); `dynamics_ensemble(...)` is the reference's constructor call and returns
whichever `dense_connect` asks for, so run.py binds it with one import:

    from amp_extensions_amd.ensemble import dynamics_ensemble as DynamicsEnsemble

Other model options (`use_resnet`, a non-ReLU activation, unequal hidden widths) raise
NotImplementedError.

`as_device_ensemble(obj)` also accepts the reference's own DynamicsEnsemble object (anything
with `models[k].model.state_dict()`, `transformations` and `threshold`), so SimEnv /
BatchedSimEnv / the costs take either.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

from .engine import AmxContext, DeviceEnsemble, flat_pairs
from .optstate import common_step, read_state, write_state

# DynamicsEnsemble's default optimizer arguments (dynamics.py:32)
DEFAULT_OPTIM_ARGS = {'optim': 'sgd', 'lr': 1e-4, 'momentum': 0.9}


def basic_mlp_layer_shapes(S: int, A: int, hidden) -> list[tuple[int, int]]:
    """(out, in) of each nn.Linear of a dense-connect BasicMLP (dynamics.py:412-420)."""
    sizes = [S + A] + list(hidden) + [S]
    return [(sizes[i + 1], sizes[i] + sum(sizes[:i])) for i in range(len(sizes) - 1)]


def plain_mlp_layer_shapes(S: int, A: int, hidden) -> list[tuple[int, int]]:
    """(out, in) of each nn.Linear of a plain BasicMLP (dense_connect=False, dynamics.py:412-420)."""
    sizes = [S + A] + list(hidden) + [S]
    return [(sizes[i + 1], sizes[i]) for i in range(len(sizes) - 1)]


class BasicMLPWeights(nn.Module):
    """Host parameter container of one BasicMLP (dynamics.py:394-420), dense-connect or plain:
    the nn.Linear layers in the reference's construction order and state-dict keys.  It has no
    forward: the member's arithmetic runs on the GPU (DeviceEnsemble)."""

    def __init__(self, input_dim: int, output_dim: int, hidden_sizes, dense_connect: bool = True):
        super().__init__()
        sizes = [input_dim] + list(hidden_sizes) + [output_dim]
        self.dense_connect = bool(dense_connect)
        self.fc_layers = nn.ModuleList(
            nn.Linear(sizes[i] + (sum(sizes[:i]) if dense_connect else 0), sizes[i + 1])
            for i in range(len(sizes) - 1))

    def layers(self):
        return [(l.weight.data, l.bias.data) for l in self.fc_layers]

    def forward(self, x):  # pragma: no cover - guard
        raise RuntimeError("BasicMLPWeights holds parameters only; forward runs on the GPU (DynamicsEnsemble)")


def _make_optimizer(params, optim_args):
    """DynamicsModel.__init__'s optimizer (dynamics.py:199-204)."""
    if optim_args['optim'] == 'sgd':
        return torch.optim.SGD(params, lr=optim_args['lr'], momentum=optim_args['momentum'], nesterov=True)
    if optim_args['optim'] == 'adam':
        return torch.optim.Adam(params, lr=optim_args['lr'], eps=optim_args['eps'])
    raise AssertionError('Use valid optimizer')


def init_model_weights(S: int, A: int, hidden, seed: int, dense_connect: bool = True):
    """DynamicsModel.__init__ RNG order: manual_seed(seed), np.random.seed(seed), then the
    BasicMLP layers constructed in order (dynamics.py:185-196, 419)."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    return [(w.clone(), b.clone()) for (w, b) in BasicMLPWeights(S + A, S, hidden, dense_connect).layers()]


def init_ensemble_weights(S: int, A: int, hidden, num_models: int = 4, base_seed: int = 100,
                          dense_connect: bool = True):
    """Member k seeded base_seed + k (dynamics.py:70-79)."""
    return [init_model_weights(S, A, hidden, base_seed + k, dense_connect) for k in range(num_models)]


def weights_from_state_dict(sd) -> list:
    """BasicMLP state_dict ('fc_layers.{i}.weight/bias') -> [(W, b), ...]."""
    n = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("fc_layers."))
    return [(sd[f"fc_layers.{i}.weight"], sd[f"fc_layers.{i}.bias"]) for i in range(n)]


class DynamicsModel:
    """models[k] of the ensemble (dynamics.py:167-392): `model` (host parameters, state-dict
    compatible), `optimizer`, `forward`, `load`, `get_state_dicts`."""

    def __init__(self, ens: "DynamicsEnsemble", k: int, state_dim: int, action_dim: int, hidden_sizes,
                 optim_args, seed: int):
        self._ens, self.k = ens, k
        self.state_dim, self.action_dim = state_dim, action_dim
        self.transform = ens.transform
        # dynamics.py:185-196: the seed, then the layers in construction order
        torch.manual_seed(seed)
        np.random.seed(seed)
        self.model = BasicMLPWeights(state_dim + action_dim, state_dim, hidden_sizes, ens.dense_connect)
        self.optimizer = _make_optimizer(self.model.parameters(), optim_args)

    def forward(self, state, action, unnormalize_out=True):
        """dynamics.py:216-233: the member's Δ (un-normalised unless unnormalize_out=False),
        returned on the ensemble's `device`.  The normalised output is recovered from the
        device's un-normalised Δ as (Δ − μ_Δ)/σ_Δ (fp32, within rounding of the reference's
        raw network output)."""
        if isinstance(state, np.ndarray):
            state = torch.from_numpy(state).float()
        if isinstance(action, np.ndarray):
            action = torch.from_numpy(action).float()
        out = self._ens.engine.model_forward(self.k, state, action)
        if not unnormalize_out and self.transform:
            mu_d, sd_d = self._ens.engine.norms[4], self._ens.engine.norms[5]
            out = (out - mu_d) / sd_d
        return out.to(self._ens.device)

    def load(self, model_state_dict, optimizer_state_dict=None):
        """dynamics.py:380-386 (the device copy is refreshed by the ensemble)."""
        self.model.load_state_dict(model_state_dict)
        if optimizer_state_dict:
            self.optimizer.load_state_dict(optimizer_state_dict)

    def get_state_dicts(self):
        """dynamics.py:388-392."""
        return {'model': self.model.state_dict(), 'optim': self.optimizer.state_dict()}

    def train(self, *a, **k):
        raise NotImplementedError("per-member training is not implemented; DynamicsEnsemble.train_on_device trains "
                                  "all members on the GPU")


def _identity_transformations(S: int, A: int):
    z_s, o_s = torch.zeros(S), torch.ones(S)
    return z_s, o_s, torch.zeros(A), torch.ones(A), z_s.clone(), o_s.clone()


def _gpu_device(gpu) -> torch.device:
    if gpu is None:
        return torch.device("cuda", torch.cuda.current_device())
    if isinstance(gpu, int):
        return torch.device("cuda", gpu)
    return torch.device(gpu)


class DynamicsEnsemble:
    """Reference-compatible DynamicsEnsemble (dynamics.py:19-165) backed by `DeviceEnsemble`."""

    def __init__(self, state_dim, action_dim, train_dataset, validate_dataset=None, num_models=4, batch_size=256,
                 hidden_sizes=[512, 512], use_resnet=False, dense_connect=True, activation='relu', transform=True,
                 optim_args=DEFAULT_OPTIM_ARGS, device=torch.device('cpu'), base_seed=100, num_workers=1, *,
                 gpu=None, ctx: AmxContext | None = None, feat_dim: int = 512, gemm: str = "f16x3"):
        """The reference's arguments (dynamics.py:20-35).  `train_dataset` supplies the
        normalizers (`get_transformations`, datasets.py:23-43) and the rows compute_threshold
        scans; `validate_dataset`, `batch_size` and `num_workers` only configure training in the
        reference and are kept for the call's shape.  Extensions (keyword-only): `gpu` (the HIP
        device the arithmetic runs on), `ctx` (share an AmxContext), `feat_dim` (the context's
        RFF width), `gemm` (DeviceEnsemble's GEMM path)."""
        if use_resnet or not dense_connect or activation != 'relu':
            raise NotImplementedError("DynamicsEnsemble implements the dense-connect ReLU BasicMLP "
                                      "(dynamics.py:394-433; run.py's --dynamic_dense_connect): got "
                                      f"use_resnet={use_resnet}, dense_connect={dense_connect}, activation={activation!r}"
                                      ".  A plain ReLU BasicMLP (dense_connect=False) is PlainDynamicsEnsemble; the "
                                      "factory dynamics_ensemble(...) returns either by dense_connect")
        self._setup(state_dim, action_dim, train_dataset, validate_dataset, num_models, batch_size, hidden_sizes,
                    True, transform, optim_args, device, base_seed, gpu, ctx, feat_dim, gemm)

    def _setup(self, state_dim, action_dim, train_dataset, validate_dataset, num_models, batch_size, hidden_sizes,
               dense_connect, transform, optim_args, device, base_seed, gpu, ctx, feat_dim, gemm):
        """The constructor's body, for either connectivity."""
        hidden_sizes = list(hidden_sizes)
        if len(hidden_sizes) < 1 or len(set(hidden_sizes)) != 1:
            raise NotImplementedError(f"the device ensemble needs equal hidden widths, got {hidden_sizes}")
        self.dense_connect = bool(dense_connect)
        self.state_dim, self.action_dim = state_dim, action_dim
        self.train_dataset, self.validate_dataset = train_dataset, validate_dataset
        self.batch_size = batch_size
        self.transformations = train_dataset.get_transformations(device) if transform else None
        self.num_models = num_models
        self.transform = transform
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        self.base_seed = base_seed
        self.hidden_sizes = hidden_sizes
        self._fit_stepped = False
        self.models = [DynamicsModel(self, k, state_dim, action_dim, hidden_sizes, optim_args, base_seed + k)
                       for k in range(num_models)]
        if ctx is None:
            ctx = AmxContext(state_dim, action_dim, n_models=num_models, hidden=hidden_sizes[0],
                             n_hidden=len(hidden_sizes), feat_dim=feat_dim, device=_gpu_device(gpu),
                             dense_connect=self.dense_connect)
        elif ctx.dense_connect != self.dense_connect:
            raise ValueError(f"the shared context is {'dense-connect' if ctx.dense_connect else 'plain'}, the "
                             f"ensemble {'dense-connect' if self.dense_connect else 'plain'}")
        self.ctx = ctx
        self.engine = DeviceEnsemble(ctx, [m.model.layers() for m in self.models], self._norms(), gemm=gemm)
        self._set_member_transformations()
        self.threshold = 0.0

    # ---- construction helpers (extensions) --------------------------------------------------
    @classmethod
    def from_weights(cls, state_dim, action_dim, weights, transformations, hidden_sizes=(512, 512, 512, 512),
                     threshold: float = 0.0, **kw):
        """An ensemble over given per-member [(W, b), ...] weights (nn.Linear layout) and the
        six normalizer vectors (datasets.py:23-43), without an offline dataset."""
        ds = _Transformations(transformations)
        ens = cls(state_dim, action_dim, ds, None, num_models=len(weights), hidden_sizes=list(hidden_sizes), **kw)
        for m, w in zip(ens.models, weights):
            with torch.no_grad():
                for lin, (W, b) in zip(m.model.fc_layers, w):
                    lin.weight.copy_(torch.as_tensor(W)), lin.bias.copy_(torch.as_tensor(b))
        ens._upload()
        ens.threshold = threshold
        return ens

    @classmethod
    def random_init(cls, state_dim, action_dim, transformations, hidden_sizes=(512, 512, 512, 512), num_models=4,
                    base_seed=100, **kw):
        """The reference's seeded init (member k: base_seed + k) with given normalizers."""
        return cls(state_dim, action_dim, _Transformations(transformations), None, num_models=num_models,
                   hidden_sizes=list(hidden_sizes), base_seed=base_seed, **kw)

    @classmethod
    def from_reference(cls, ref, **kw):
        """Convert the reference's DynamicsEnsemble object (its members' BasicMLP state dicts,
        transformations and threshold)."""
        sds = [m.model.state_dict() for m in ref.models]
        w = [weights_from_state_dict(sd) for sd in sds]
        S, A = ref.state_dim, ref.action_dim
        hidden = [W.shape[0] for (W, _) in w[0][:-1]]
        tr = ref.transformations if getattr(ref, "transform", True) and ref.transformations is not None \
            else _identity_transformations(S, A)
        return cls.from_weights(S, A, w, tr, hidden_sizes=hidden, threshold=float(ref.threshold), **kw)

    # ---- the reference surface -------------------------------------------------------------
    def _norms(self):
        if self.transformations is None:
            return _identity_transformations(self.state_dim, self.action_dim)
        return tuple(torch.as_tensor(x).detach().float().cpu() for x in self.transformations)

    def _set_member_transformations(self):
        if self.transform:  # dynamics.py:128-131
            for m in self.models:
                (m.state_mean, m.state_scale, m.action_mean, m.action_scale, m.diff_mean,
                 m.diff_scale) = self.transformations

    def _upload(self):
        self.engine.set_weights([m.model.layers() for m in self.models])

    @property
    def threshold(self) -> float:
        return self.engine.threshold

    @threshold.setter
    def threshold(self, v) -> None:
        self.engine.threshold = float(v)

    def train(self, *a, **k):
        raise NotImplementedError("DynamicsEnsemble.train is not bound; call train_on_device (the same arguments and "
                                  "return value, all members trained on the GPU)")

    # ---- training on the device (dynamics.py:82-108, 236-378) ------------------------------
    def _optimizer_config(self):
        """(optim, lr, p1) of the members' optimizers (the loaded checkpoint's param_groups
        included); anything the device step does not implement raises."""
        cfg = None
        for m in self.models:
            kind, pg, _ = read_state(m.optimizer)
            if kind == "adam":
                if tuple(pg["betas"]) != (0.9, 0.999) or pg["weight_decay"] != 0:
                    raise NotImplementedError(f"Adam options {pg['betas']}, weight_decay={pg['weight_decay']}, "
                                              f"amsgrad={pg['amsgrad']} (supported: torch's defaults with lr, eps)")
                c = ("adam", float(pg["lr"]), float(pg["eps"]))
            else:
                if not pg["nesterov"] or pg["weight_decay"] != 0:
                    raise NotImplementedError("SGD options (supported: momentum with nesterov=True, dampening 0)")
                c = ("sgd", float(pg["lr"]), float(pg["momentum"]))
            if cfg is not None and c != cfg:
                raise NotImplementedError("members with different optimizer settings")
            cfg = c
        return cfg

    def _host_opt_state(self):
        """The members' optimizer state in DeviceEnsemble.fit_begin's form."""
        out = []
        for m in self.models:
            _, _, states = read_state(m.optimizer)
            pairs = lambda j: [(states[i][j], states[i + 1][j]) for i in range(0, len(states), 2)]  # noqa: E731
            out.append({"step": common_step(states), "s1": pairs(1), "s2": pairs(2)})
        return out

    def sync_to_host(self):
        """Copy the device master weights and optimizer state into `models[k].model` and
        `models[k].optimizer` (exp_avg / exp_avg_sq / step, or momentum_buffer, in torch's
        layout), so save_ensemble writes a reference-format checkpoint.  Needs an open
        training state (it is called by train_on_device)."""
        optim = self.engine._fit["optim"]
        weights, opt = self.engine.fit_state()
        with torch.no_grad():
            for m, w, st in zip(self.models, weights, opt):
                for i, lin in enumerate(m.model.fc_layers):
                    lin.weight.copy_(w[i][0]), lin.bias.copy_(w[i][1])
                if not self._fit_stepped and st["step"] == 0:
                    continue
                L = len(w) - 1
                write_state(m.optimizer, optim, st["step"], flat_pairs(st["s1"], L), flat_pairs(st["s2"], L))

    def train_on_device(self, epochs, validate=False, logger=None, log_epoch=False, grad_clip=0, save_path=None,
                        save_checkpoints=False, writer=None):
        """DynamicsEnsemble.train (dynamics.py:82-108) with DynamicsModel.train's loop
        (:305-378) on the GPU: the same arguments, log strings, `writer.add_scalar` calls,
        `save_path` files and return value ([(train_min_loss, train_losses[0]) per member]).

        All members advance in the same launches, each on the index batches the reference's
        member-major DataLoader iterations would have drawn from torch's global generator
        (plan_batches); the generator is left in the state after the reference's last draw.
        Log lines therefore arrive epoch by epoch for all members rather than member by member.
        As in the reference on current torch, the "best" state dicts are views of the live
        tensors, so the members end with the last epoch's parameters.  Optimizer state loaded
        by load_ensemble is uploaded first (training resumes a checkpoint); afterwards the host
        members hold the trained parameters and optimizer state and the inference limb images
        are refreshed in place.  `threshold` is left for compute_threshold()."""
        assert (not validate) or (validate and self.validate_dataset)
        epochs = int(epochs)
        if not grad_clip:
            grad_clip = 0.0
        if grad_clip < 0:
            raise ValueError(f"grad_clip={grad_clip}")
        optim, lr, p1 = self._optimizer_config()
        tr = _dataset_tensors(self.train_dataset)
        va = _dataset_tensors(self.validate_dataset) if validate else None
        M, bs = self.num_models, int(self.batch_size)
        eng = self.engine
        eng.fit_begin(tr, optim, lr, p1, bs, val_data=va, opt_state=self._host_opt_state(), num_models=M,
                      hidden_sizes=self.hidden_sizes)
        self._fit_stepped = False
        try:
            return self._train_loop(epochs, validate, logger, log_epoch, float(grad_clip), save_path,
                                    save_checkpoints, writer, tr[0].shape[0], va[0].shape[0] if validate else 0)
        finally:
            eng.fit_end()

    def _train_loop(self, epochs, validate, logger, log_epoch, grad_clip, save_path, save_checkpoints, writer,
                    n_train, n_val):
        M, bs, eng = self.num_models, int(self.batch_size), self.engine
        plan, final_rng = plan_batches(n_train, n_val, bs, epochs, M, validate)
        train_loader = index_loader(n_train, bs)
        val_loader = index_loader(n_val, bs) if validate else None
        paths = [None] * M
        for i in range(M):
            if logger is not None:
                logger.info(f'>>>>Training Model {i+1}/{self.num_models}')
            if save_path is not None:
                paths[i] = os.path.join(save_path, f'model{i}')
                if not os.path.exists(paths[i]):
                    os.mkdir(paths[i])
        inf = float('inf')
        t_min, t_min_ep, t_losses = [inf] * M, [inf] * M, [[] for _ in range(M)]
        v_min, v_min_ep, v_losses = [inf] * M, [inf] * M, [[] for _ in range(M)]
        last_avg = [None] * M

        def gather(loader, which, epoch):
            per = [materialise(loader, plan[g][epoch][which]) for g in range(M)]
            sizes = [len(b) for b in per[0]]
            idx = np.zeros((M, len(sizes), bs), dtype=np.int32)
            for g in range(M):
                for s_, b in enumerate(per[g]):
                    idx[g, s_, :len(b)] = b
            return idx, sizes

        for epoch in range(epochs):
            idx, sizes = gather(train_loader, 0, epoch)
            losses = eng.fit_epoch(idx, sizes, train=True, grad_clip=grad_clip)
            self._fit_stepped = True
            ckpt = save_path is not None and save_checkpoints and ((epoch + 1) % 100 == 0 or (epoch + 1) == epochs // 2)
            if ckpt:
                self.sync_to_host()
            for g in range(M):
                avg = np.average([float(x) for x in losses[g]])
                last_avg[g] = avg
                if ckpt:
                    m = self.models[g]
                    torch.save({'model': m.model.state_dict(), 'optim': m.optimizer.state_dict(), 'epoch': epoch + 1,
                                'loss': avg}, os.path.join(paths[g], f'{epoch + 1}_checkpoint.pt'))
                if logger is not None:
                    if log_epoch:
                        logger.info('Epoch: {}, Train Loss: {}'.format(epoch, avg))
                else:
                    print('Epoch {} Train Loss: {}'.format(epoch, avg))
                t_losses[g].append(avg)
                if writer is not None:
                    writer.add_scalar("Loss/train", avg, epoch)
                if avg < t_min[g]:
                    t_min_ep[g], t_min[g] = epoch, avg
            if validate:
                idx, sizes = gather(val_loader, 1, epoch)
                losses = eng.fit_epoch(idx, sizes, train=False, split="val")
                for g in range(M):
                    avg = np.average([float(x) for x in losses[g]])
                    if logger is not None:
                        if log_epoch:
                            logger.info('Epoch {} Validation Loss: {}'.format(epoch, avg))
                    else:
                        print('Epoch {} Validation Loss: {}'.format(epoch, avg))
                    v_losses[g].append(avg)
                    if writer is not None:
                        writer.add_scalar("Loss/validate", avg, epoch)
                    if avg < v_min[g]:
                        v_min_ep[g], v_min[g] = epoch, avg
        torch.set_rng_state(final_rng)
        self.sync_to_host()
        eng.fit_refresh()
        info = []
        for g, m in enumerate(self.models):
            if save_path is not None:
                # the reference's "best" dicts are state_dict() views of the live tensors: all
                # three files hold the final parameters, under the best epoch's number and loss
                sd = lambda: {'model': m.model.state_dict(), 'optim': m.optimizer.state_dict()}
                torch.save({**sd(), 'epoch': epochs, 'loss': last_avg[g]}, os.path.join(paths[g], 'final_model.pt'))
                torch.save({**sd(), 'epoch': t_min_ep[g] + 1, 'loss': t_min[g]},
                           os.path.join(paths[g], 'best_train_checkpoint.pt'))
                if validate:
                    torch.save({**sd(), 'epoch': v_min_ep[g] + 1, 'loss': v_min[g]},
                               os.path.join(paths[g], 'best_validate_checkpoint.pt'))
            if logger is not None:
                logger.info('Train: Dynamics Start | Best Loss | Epoch: {} | {} | {}'.format(
                    t_losses[g][0], t_min[g], t_min_ep[g]))
                if validate:
                    logger.info('Validate: Dynamics Start | Best Loss | Epoch: {} | {} | {}'.format(
                        v_losses[g][0], v_min[g], v_min_ep[g]))
            info.append((t_min[g], t_losses[g][0]))
        return info

    def save_ensemble(self, save_path):
        """dynamics.py:110-116: a list of {'model', 'optim'} state dicts."""
        torch.save([m.get_state_dicts() for m in self.models], save_path)

    def load_ensemble(self, state_dict_path):
        """dynamics.py:118-131: the members' model (and optimizer) state dicts from the list
        save_ensemble wrote, then the dataset's transformations; the device weights are
        refreshed in place.  Loaded with the weights-only unpickler (tensors and plain
        containers; anything else in the file is refused)."""
        state_dicts = torch.load(state_dict_path, map_location="cpu", weights_only=True)
        assert len(state_dicts) == len(self.models)
        print("loading ensemble")
        for model, state_dict in zip(self.models, state_dicts):
            model.load(state_dict['model'], state_dict['optim'])
        print("Done loading ensemble")
        self._set_member_transformations()
        self._upload()

    def discrepancy_device(self, state, action) -> torch.Tensor:
        """The per-row max pairwise disagreement, left on the GPU (the costs' input)."""
        return self.engine.get_action_discrepancy(torch.as_tensor(state), torch.as_tensor(action))

    def compute_discrepancy(self, state, action):
        """dynamics.py:134-143: max over member pairs of ‖pred_i − pred_j‖₂, on the CPU."""
        return self.discrepancy_device(state, action).to(torch.device('cpu'))

    def get_action_discrepancy(self, state, action):
        """dynamics.py:154-165 (float32 inputs; the result on the CPU as the reference's)."""
        return self.compute_discrepancy(state, action)

    def compute_threshold(self, states=None, actions=None):
        """dynamics.py:145-152: the max disagreement over the whole offline (train) dataset.
        (states, actions) may be given explicitly (extension; then the threshold is returned)."""
        explicit = states is not None
        if not explicit:
            ds = self.train_dataset
            if hasattr(ds, "states") and hasattr(ds, "actions"):
                states, actions = ds.states, ds.actions
            else:
                rows = [ds[i] for i in range(len(ds))]
                states = torch.stack([r[0] for r in rows])
                actions = torch.stack([r[1] for r in rows])
        dev = self.ctx.device
        self.engine.compute_threshold(torch.as_tensor(states).to(dev).float(), torch.as_tensor(actions).to(dev).float())
        return self.threshold if explicit else None


class PlainDynamicsEnsemble(DynamicsEnsemble):
    """The reference's DynamicsEnsemble with plain members (dense_connect=False, run.py without
    --dynamic_dense_connect; --dynamic_hidden_sizes defaults to [1024, 1024]): layer i reads
    layer i-1's output only (dynamics.py:412-433).  Everything else is DynamicsEnsemble's: the
    members' state dicts and checkpoints in the reference's format, the threshold and
    discrepancy calls, train_on_device / sync_to_host, from_weights / random_init /
    from_reference, and the raising train()."""

    def __init__(self, state_dim, action_dim, train_dataset, validate_dataset=None, num_models=4, batch_size=256,
                 hidden_sizes=[512, 512], use_resnet=False, dense_connect=False, activation='relu', transform=True,
                 optim_args=DEFAULT_OPTIM_ARGS, device=torch.device('cpu'), base_seed=100, num_workers=1, *,
                 gpu=None, ctx: AmxContext | None = None, feat_dim: int = 512, gemm: str = "f16x3"):
        if dense_connect:
            raise ValueError("PlainDynamicsEnsemble is the dense_connect=False ensemble; dense-connect members are "
                             "DynamicsEnsemble (or call the factory dynamics_ensemble(...))")
        if use_resnet or activation != 'relu':
            raise NotImplementedError("the device ensemble implements the ReLU BasicMLP (dynamics.py:394-433): got "
                                      f"use_resnet={use_resnet}, activation={activation!r}")
        self._setup(state_dim, action_dim, train_dataset, validate_dataset, num_models, batch_size, hidden_sizes,
                    False, transform, optim_args, device, base_seed, gpu, ctx, feat_dim, gemm)


def dynamics_ensemble(state_dim, action_dim, train_dataset, validate_dataset=None, num_models=4, batch_size=256,
                      hidden_sizes=[512, 512], use_resnet=False, dense_connect=False, activation='relu',
                      transform=True, optim_args=DEFAULT_OPTIM_ARGS, device=torch.device('cpu'), base_seed=100,
                      num_workers=1, **kw):
    """The reference's DynamicsEnsemble(...) call (dynamics.py:20-35) with run.py's default for
    its store_true flag, dense_connect=False: a DynamicsEnsemble when dense_connect, else a
    PlainDynamicsEnsemble.
    Keyword extensions (gpu, ctx, feat_dim, gemm) pass through."""
    cls = DynamicsEnsemble if dense_connect else PlainDynamicsEnsemble
    return cls(state_dim, action_dim, train_dataset, validate_dataset, num_models=num_models, batch_size=batch_size,
               hidden_sizes=hidden_sizes, use_resnet=use_resnet, dense_connect=dense_connect, activation=activation,
               transform=transform, optim_args=optim_args, device=device, base_seed=base_seed,
               num_workers=num_workers, **kw)


def _dataset_tensors(ds):
    """(states, actions, next_states) of an AmpDataset-like dataset (its tensors, or its rows)."""
    if all(hasattr(ds, k) for k in ("states", "actions", "next_states")):
        return ds.states, ds.actions, ds.next_states
    rows = [ds[i] for i in range(len(ds))]
    return tuple(torch.stack([r[j] for r in rows]) for j in range(3))


# ---- the reference's batch orders ----------------------------------------------------------
# DynamicsModel.train iterates DataLoader(shuffle=True) objects that draw from torch's global
# generator, member-major: member 0's epochs (each followed by a validation-loader iteration
# under `validate`), then member 1's, ...  The draws do not depend on training results, so the
# order is replayed with real DataLoaders over an index dataset: consumption of the generator
# equals the installed torch's by construction.


class _IndexDataset(Dataset):
    """Row i is the index i; a batch is the list of its indices."""

    def __init__(self, n: int):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i

    def __getitems__(self, idx):
        return idx


def _identity(batch):
    return batch


def index_loader(n: int, batch_size: int) -> DataLoader:
    """DataLoader(shuffle=True, drop_last=False) over the indices 0..n-1."""
    return DataLoader(_IndexDataset(n), batch_size=batch_size, shuffle=True, collate_fn=_identity)


def plan_batches(n_train: int, n_val: int, batch_size: int, epochs: int, num_models: int, validate: bool):
    """Walk the reference's (member, epoch[, val]) loader iterations in its order and record
    torch.get_rng_state() before each one: returns (plan, final_state) with plan[g][e] =
    (state before the train iteration, state before the validation iteration or None).  An
    iteration's draws from the global generator all happen by its first batch, so each is
    advanced by one batch only; no permutation is kept.  The global generator ends in
    final_state."""
    train_loader = index_loader(n_train, batch_size)
    val_loader = index_loader(n_val, batch_size) if validate else None
    plan = []
    for _ in range(num_models):
        rows = []
        for _ in range(epochs):
            st = torch.get_rng_state()
            next(iter(train_loader))
            sv = None
            if validate:
                sv = torch.get_rng_state()
                next(iter(val_loader))
            rows.append((st, sv))
        plan.append(rows)
    return plan, torch.get_rng_state()


def materialise(loader: DataLoader, rng_state) -> list:
    """The index batches of the loader iteration that starts from `rng_state`."""
    torch.set_rng_state(rng_state)
    return [list(map(int, b)) for b in loader]


class _Transformations:
    """A stand-in train_dataset that only supplies get_transformations (from_weights / random_init)."""

    def __init__(self, tr):
        self._tr = tuple(torch.as_tensor(x).detach().float().cpu() for x in tr)

    def get_transformations(self, device=None):
        return tuple(x.to(device) if device is not None else x for x in self._tr)

    def __len__(self):
        return 0


def as_device_ensemble(ens) -> DeviceEnsemble:
    """The DeviceEnsemble behind `ens`: this package's DynamicsEnsemble, a DeviceEnsemble, or
    the reference's DynamicsEnsemble object (converted once and cached on it; run.py loads the
    weights before it builds the env, run.py:78-120)."""
    if isinstance(ens, DeviceEnsemble):
        return ens
    if isinstance(ens, DynamicsEnsemble):
        return ens.engine
    conv = getattr(ens, "_amx_ensemble", None)
    if conv is None:
        if not (hasattr(ens, "models") and hasattr(ens, "threshold")):
            raise TypeError(f"expected a DynamicsEnsemble, got {type(ens).__name__}")
        # the members' own flag (BasicMLP.dense_connect, dynamics.py:409); an object without one is dense
        dense = bool(getattr(getattr(ens.models[0], "model", None), "dense_connect", True))
        conv = (DynamicsEnsemble if dense else PlainDynamicsEnsemble).from_reference(ens)
        try:
            ens._amx_ensemble = conv
        except AttributeError:
            pass
    return conv.engine
