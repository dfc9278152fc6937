"""The reference's ensemble-training loop restated in torch on the CPU (the comparator of
test_gpu_efit.py and tools/efit_time.py): a module with BasicMLP's dense-connect forward
(milo/milo/dynamics.py:394-433), torch.optim.Adam / SGD(nesterov=True), nn.MSELoss,
clip_grad_norm_ (DynamicsModel.train_step, dynamics.py:236-250) and injected index batches.
It runs in fp64 (the yardstick) or fp32."""
import numpy as np
import torch
import torch.nn as nn


def synthetic_transitions(n, S, A, seed, power=1):
    """Seeded (s, a, s') float32 tensors with a learnable delta: s' = s + 0.05 tanh([s, a] Q) + noise.
    power > 1 gives heavy-tailed states and actions (z^power): larger normalised inputs and
    first-step gradient norms."""
    rs = np.random.RandomState(seed)
    s = 0.5 * rs.randn(n, S) ** power
    a = rs.randn(n, A) ** power
    Q = rs.randn(S + A, S) / np.sqrt(S + A)
    s2 = s + 0.05 * np.tanh(np.concatenate([s, a], 1) @ Q) + 0.01 * rs.randn(n, S)
    return tuple(torch.from_numpy(x).float() for x in (s, a, s2))


class DenseMLP(nn.Module):
    def __init__(self, S, A, hidden):
        super().__init__()
        sizes = [S + A] + list(hidden) + [S]
        self.fc_layers = nn.ModuleList(nn.Linear(sizes[i] + sum(sizes[:i]), sizes[i + 1])
                                       for i in range(len(sizes) - 1))

    def forward(self, x):
        for fc in self.fc_layers[:-1]:
            x = torch.cat([x, torch.relu(fc(x))], dim=1)
        return self.fc_layers[-1](x)


def make_optimizer(params, optim, lr, p1):
    if optim == "adam":
        return torch.optim.Adam(params, lr=lr, eps=p1)
    return torch.optim.SGD(params, lr=lr, momentum=p1, nesterov=True)


def restate_member(state_dict, opt_state_dict, norms, data, events, optim, lr, p1, grad_clip, dtype):
    """One member through `events` = [('t' | 'v', data split, index array), ...] in order.
    `data` = {'train': (s, a, s'), 'val': ...}; `norms` the six transformation vectors or None.
    Returns dict(model=state_dict, optim=optimizer.state_dict(), losses=[(kind, loss)],
    first_norm=the first train step's gradient norm before clipping)."""
    S, A = data["train"][0].shape[1], data["train"][1].shape[1]
    hidden = [state_dict[f"fc_layers.{i}.weight"].shape[0] for i in range(len(state_dict) // 2 - 1)]
    net = DenseMLP(S, A, hidden)
    net.load_state_dict(state_dict)
    opt = make_optimizer(net.parameters(), optim, lr, p1)
    if opt_state_dict is not None:
        opt.load_state_dict(opt_state_dict)
    net = net.to(dtype)  # after load_state_dict: the optimizer state follows the parameters' dtype below
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


def events_from_plan(plan_g, train_loader, val_loader, materialise):
    """The ('t' | 'v', split, idx) events of one member from plan_batches' rows."""
    ev = []
    for st, sv in plan_g:
        ev += [("t", "train", b) for b in materialise(train_loader, st)]
        if sv is not None:
            ev += [("v", "val", b) for b in materialise(val_loader, sv)]
    return ev
