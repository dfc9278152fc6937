"""Where the device fits keep their parameters, and how torch.optim state gets there and back.

Every learner that trains on the device (the value baseline, the discriminator, the policy under
BC / PPO, the dynamics ensemble) holds its optimizer state in flat fp32 vectors whose entries are
the nn.Linear tensors in torch's parameter order, zero-padded to the kernels' tile sizes.
`ParamLayout` is that description, once; `read_state` / `write_state` are the one path between
a torch.optim.Adam / SGD (or its state_dict) and those vectors.  Host code only: torch and numpy.
"""
from __future__ import annotations

from math import prod

import numpy as np
import torch

STATE_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer", None)}


class ParamLayout:
    """Entries `(padded_shape, live_shape[, cols])` in torch's parameter order, laid end to end.
    The live tensor occupies the leading block of its padded one; `cols` (integer indices) sends
    live input column j to padded column cols[j] instead."""

    def __init__(self, entries):
        self.padded, self.live, self.offsets, self._index = [], [], [], []
        o = 0
        for pad, live, *cols in entries:
            pad, live = tuple(int(n) for n in pad), tuple(int(n) for n in live)
            index = [slice(0, n) for n in live]
            reach = live
            if cols and cols[0] is not None:
                index[-1] = torch.as_tensor(np.asarray(cols[0]), dtype=torch.int64)
                reach = live[:-1] + (int(index[-1].max()) + 1,)
                assert index[-1].numel() == live[-1]
            assert len(pad) == len(live) and all(r <= p for r, p in zip(reach, pad))
            self.padded.append(pad)
            self.live.append(live)
            self.offsets.append(o)
            self._index.append((Ellipsis,) + tuple(index))
            o += prod(pad)
        self.size = o  # the P of amx_*_param_count

    def views(self, flat: torch.Tensor):
        """Per-entry padded views of a [size] or [M][size] tensor (any device, no copy)."""
        if flat.shape[-1] != self.size:
            raise ValueError(f"expected a last dimension of {self.size}, found shape {tuple(flat.shape)}")
        return [flat[..., o:o + prod(pad)].unflatten(-1, pad) for o, pad in zip(self.offsets, self.padded)]

    def pack(self, tensors) -> torch.Tensor:
        """Live tensors -> host fp32 [size], zero outside the live entries."""
        tensors = [torch.as_tensor(t) for t in tensors]
        found = [tuple(t.shape) for t in tensors]
        if found != self.live:
            raise ValueError(f"expected tensors of shapes {self.live}, found {found}")
        flat = torch.zeros(self.size, dtype=torch.float32)
        for v, index, t in zip(self.views(flat), self._index, tensors):
            v[index] = t.detach().float().cpu()
        return flat

    def unpack(self, flat: torch.Tensor):
        """[size] -> the live tensors (clones)."""
        return [v[index].clone() for v, index in zip(self.views(flat), self._index)]

    def live_mask(self) -> torch.Tensor:
        mask = torch.zeros(self.size, dtype=torch.bool)
        for v, index in zip(self.views(mask), self._index):
            v[index] = True
        return mask


def _mlp_entries(k, k_pad, widths, padded, head_bias_pad):
    out = []
    for h, hp in zip(widths, padded):
        out += [((hp, k_pad), (h, k)), ((hp,), (h,))]
        k, k_pad = h, hp
    return out + [((1, k_pad), (1, k)), ((head_bias_pad,), (1,))]


def baseline_layout(k: int, kf: int, widths, padded) -> ParamLayout:
    """The value baseline (amx_vfit_param_count): k = S + 4 features padded to kf, hidden `widths`
    padded to `padded`, a scalar head."""
    return ParamLayout(_mlp_entries(k, kf, widths, padded, 1))


def disc_layout(D: int, Dp: int, widths, padded) -> ParamLayout:
    """The discriminator (amx_dfit_param_count): as the baseline's, the head's bias padded to 4."""
    return ParamLayout(_mlp_entries(D, Dp, widths, padded, 4))


def policy_layout(S: int, A: int, hidden=(32, 32)) -> ParamLayout:
    """The policy's theta (amx_npg_param_count): W1, b1, W2, b2, W3, b3, log_std, unpadded."""
    h0, h1 = hidden
    shapes = [(h0, S), (h0,), (h1, h0), (h1,), (A, h1), (A,), (A,)]
    return ParamLayout([(s, s) for s in shapes])


def ensemble_layout(S: int, A: int, hidden: int, L: int, k0_pad: int, Hp: int, ldk: int, n_out_pad: int) -> ParamLayout:
    """One member of the dense-connect ensemble (amx_efit_param_count): W_i [Hp][k0_pad + i Hp],
    b_i [Hp] per hidden layer, then W_out [n_out_pad][ldk], b_out; nn.Linear input column j lives
    in column cols[j] of the dense-concat activation row [s, a, pad | h0 | h1 | ...]."""
    cols = np.concatenate([np.arange(S + A)] + [k0_pad + i * Hp + np.arange(hidden) for i in range(L)])
    entries = []
    for i in range(L + 1):
        n, k = (n_out_pad, ldk) if i == L else (Hp, k0_pad + i * Hp)
        rows, n_in = S if i == L else hidden, S + A + i * hidden
        entries += [((n, k), (rows, n_in), cols[:n_in]), ((n,), (rows,))]
    return ParamLayout(entries)


def plain_ensemble_layout(S: int, A: int, hidden: int, L: int, k0_pad: int, Hp: int, n_out_pad: int) -> ParamLayout:
    """One member of the plain (dense_connect=False) ensemble (amx_efit_param_count of a plain
    context): W_0 [Hp][k0_pad], then W_i [Hp][Hp] per further hidden layer and W_out
    [n_out_pad][Hp], each followed by its bias.  A layer's input columns are those of the one
    window it reads, so the live block is the leading one."""
    entries = []
    for i in range(L + 1):
        n, k = (n_out_pad if i == L else Hp), (k0_pad if i == 0 else Hp)
        rows, n_in = (S if i == L else hidden), (S + A if i == 0 else hidden)
        entries += [((n, k), (rows, n_in)), ((n,), (rows,))]
    return ParamLayout(entries)


# ---- torch.optim state ------------------------------------------------------------------------

def read_state(optimizer, kinds=("adam", "sgd")):
    """A torch.optim.Adam / SGD, or the state_dict() of one -> (kind, hyper, states): kind "adam"
    or "sgd", hyper the one parameter group's settings, states[i] = (step, s1, s2) of the group's
    i-th parameter: (step, exp_avg, exp_avg_sq), (0, momentum_buffer, None), or (0, None, None)
    for a parameter without state.  Refuses what no device optimizer implements."""
    is_dict = isinstance(optimizer, dict)
    groups, state = (optimizer["param_groups"], optimizer["state"]) if is_dict else \
        (optimizer.param_groups, optimizer.state)
    if len(groups) != 1:
        raise NotImplementedError(f"the device fit supports one parameter group, not {len(groups)}")
    hyper = {k: v for k, v in groups[0].items() if k != "params"}
    if is_dict:  # a state_dict carries no type: the group's keys tell Adam and SGD from the rest
        kind = "adam" if {"betas", "amsgrad"} <= hyper.keys() else "sgd" if {"nesterov"} <= hyper.keys() else None
    else:
        kind = {torch.optim.Adam: "adam", torch.optim.SGD: "sgd"}.get(type(optimizer))
    if kind not in kinds:
        name = "this state_dict's optimizer" if is_dict else type(optimizer).__name__
        raise NotImplementedError(f"the device fit implements torch.optim {' / '.join(kinds)}, not {name}")
    refused = [k for k in ("amsgrad", "maximize", "dampening", "decoupled_weight_decay") if hyper.get(k)]
    if refused:  # (decoupled_weight_decay: an AdamW's state_dict, which has Adam's keys)
        raise NotImplementedError(f"the device fit does not implement {', '.join(refused)}")
    k1, k2 = STATE_KEYS[kind]
    states = []
    for p in groups[0]["params"]:
        st = state.get(p) or {}
        if st.get(k1) is None:
            states.append((0, None, None))
        else:
            states.append((int(float(st["step"])) if k2 else 0, st[k1], st[k2] if k2 else None))
    return kind, hyper, states


def common_step(states) -> int:
    """The one step count of `states`: the parameters that carry state must agree on it."""
    steps = {step for step, s1, _ in states if s1 is not None}
    if len(steps) > 1:
        raise NotImplementedError(f"the parameters are at different optimizer steps {sorted(steps)}")
    return steps.pop() if steps else 0


def pack_state(layout: ParamLayout, kind: str, states):
    """states (read_state's) -> (s1 [size], s2 [size] or None for SGD), host fp32; parameters
    without state load as zeros."""
    if len(states) != len(layout.live):
        raise ValueError(f"optimizer holds {len(states)} parameters, the model has {len(layout.live)}")
    pick = lambda j: layout.pack([torch.zeros(live) if st[j] is None else st[j]  # noqa: E731
                                  for st, live in zip(states, layout.live)])
    return pick(1), pick(2) if kind == "adam" else None


def write_state(optimizer, kind: str, step: int, s1, s2=None) -> None:
    """Per-parameter tensors s1 (and s2 for Adam) at `step` -> optimizer.state of the group's
    leading len(s1) parameters, in torch's own form.  Nothing is written unless everything fits."""
    k1, k2 = STATE_KEYS[kind]
    new = []
    for p, *state in zip(optimizer.param_groups[0]["params"], s1, *([s2] if k2 else [])):
        if any(t.numel() != p.numel() for t in state):
            raise ValueError(f"expected state of shape {tuple(p.shape)}, found {tuple(state[0].shape)}")
        st = {"step": torch.tensor(float(step), dtype=torch.float32)} if k2 else {}
        st.update({k: t.to(p.device).view_as(p) for k, t in zip((k1, k2), state)})
        new.append((p, st))
    for p, st in new:
        optimizer.state[p] = st
