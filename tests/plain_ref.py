"""The plain (dense_connect=False) BasicMLP of the reference restated in torch on the CPU
(milo/milo/dynamics.py:394-433: layer i reads layer i-1's output only), with
DynamicsModel.forward's normalisation (:216-233) and DynamicsModel.train_step (:236-250):
the comparator of test_cpu_plain.py / test_gpu_plain.py and of tools/efit_time.py --plain.  It
runs in fp64 (the yardstick) or fp32 (what the reference's own torch forward computes)."""
import numpy as np
import torch
import torch.nn as nn

from efit_ref import make_optimizer


def plain_layer_shapes(S, A, hidden):
    """(out, in) of each nn.Linear of BasicMLP(S + A, S, hidden, dense_connect=False)."""
    sizes = [S + A] + list(hidden) + [S]
    return [(sizes[i + 1], sizes[i]) for i in range(len(sizes) - 1)]


class PlainMLP(nn.Module):
    def __init__(self, S, A, hidden):
        super().__init__()
        self.fc_layers = nn.ModuleList(nn.Linear(k, n) for n, k in plain_layer_shapes(S, A, hidden))

    def forward(self, x):
        for fc in self.fc_layers[:-1]:
            x = torch.relu(fc(x))
        return self.fc_layers[-1](x)


def hidden_of(state_dict):
    return [state_dict[f"fc_layers.{i}.weight"].shape[0] for i in range(len(state_dict) // 2 - 1)]


def init_weights(S, A, hidden, seed):
    """DynamicsModel.__init__'s seeded construction (dynamics.py:185-196) of a plain member:
    [(W, b), ...] in nn.Linear layout."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    return [(l.weight.data.clone(), l.bias.data.clone()) for l in PlainMLP(S, A, hidden).fc_layers]


def load_net(weights_or_sd, S, A, dtype):
    if isinstance(weights_or_sd, dict):
        sd = weights_or_sd
    else:
        sd = {}
        for i, (W, b) in enumerate(weights_or_sd):
            sd[f"fc_layers.{i}.weight"], sd[f"fc_layers.{i}.bias"] = torch.as_tensor(W), torch.as_tensor(b)
    net = PlainMLP(S, A, hidden_of(sd))
    net.load_state_dict(sd)
    return net.to(dtype)


def forward(weights_or_sd, norms, s, a, dtype=torch.float64, unnormalize=True, layers=False):
    """One member's DynamicsModel.forward: the un-normalised (or raw) delta of rows (s, a) in
    `dtype`; layers=True also returns every hidden layer's output."""
    s, a = torch.as_tensor(s).float().to(dtype), torch.as_tensor(a).float().to(dtype)
    net = load_net(weights_or_sd, s.shape[1], a.shape[1], dtype)
    nr = None if norms is None else [torch.as_tensor(x).float().to(dtype) for x in norms]
    if nr is not None:
        s, a = (s - nr[0]) / nr[1], (a - nr[2]) / nr[3]
    with torch.no_grad():
        x = torch.cat([s, a], 1)
        hs = []
        for fc in net.fc_layers[:-1]:
            x = torch.relu(fc(x))
            hs.append(x)
        out = net.fc_layers[-1](x)
        if nr is not None and unnormalize:
            out = (out * nr[5]) + nr[4]
    return (out, hs) if layers else out


def disagreement(preds):
    """compute_discrepancy (dynamics.py:134-143): max over member pairs of the rows' L2 distance."""
    M = preds.shape[0]
    d = torch.stack([torch.norm(preds[i] - preds[j], p=2, dim=1) for i in range(M) for j in range(i + 1, M)])
    return d.max(0).values


def restate_member(state_dict, opt_state_dict, norms, data, events, optim, lr, p1, grad_clip, dtype):
    """efit_ref.restate_member for a plain member: `events` = [('t' | 'v', split, index array), ...]
    in order through DynamicsModel.train_step / validate_step.  Returns dict(model, optim, losses,
    first_norm)."""
    S, A = data["train"][0].shape[1], data["train"][1].shape[1]
    net = PlainMLP(S, A, hidden_of(state_dict))
    net.load_state_dict(state_dict)
    opt = make_optimizer(net.parameters(), optim, lr, p1)
    if opt_state_dict is not None:
        opt.load_state_dict(opt_state_dict)
    net = net.to(dtype)
    for st in opt.state.values():
        for k, v in st.items():
            if torch.is_tensor(v) and k != "step":
                st[k] = v.to(dtype)
    dat = {k: tuple(x.float().to(dtype) for x in v) for k, v in data.items()}
    nr = None if norms is None else [torch.as_tensor(x).float().to(dtype) for x in norms]
    loss_fn = nn.MSELoss()
    losses, first_norm = [], None
    for kind, split, idx in events:
        s, a, s2 = [x[torch.as_tensor(np.asarray(idx), dtype=torch.long)] for x in dat[split]]
        target = s2 - s
        if nr is not None:
            s, a, target = (s - nr[0]) / nr[1], (a - nr[2]) / nr[3], (target - nr[4]) / nr[5]
        if kind == "v":
            with torch.no_grad():
                losses.append(("v", loss_fn(net(torch.cat([s, a], 1)), target).item()))
            continue
        opt.zero_grad()
        loss = loss_fn(net(torch.cat([s, a], 1)), target)
        loss.backward()
        if first_norm is None:
            first_norm = float(torch.norm(torch.stack([p.grad.norm(2) for p in net.parameters()]), 2))
        if grad_clip:
            nn.utils.clip_grad_norm_(net.parameters(), grad_clip)
        opt.step()
        losses.append(("t", loss.item()))
    return dict(model=net.state_dict(), optim=opt.state_dict(), losses=losses, first_norm=first_norm)


def train_step(state_dict, norms, batch, optim, lr, p1, grad_clip, dtype=torch.float64):
    """One DynamicsModel.train_step of a fresh optimizer on `batch` = (s, a, s'): (loss, the
    updated state dict)."""
    n = batch[0].shape[0]
    r = restate_member(state_dict, None, norms, {"train": batch}, [("t", "train", np.arange(n))], optim, lr, p1,
                       grad_clip, dtype)
    return r["losses"][0][1], r["model"]
