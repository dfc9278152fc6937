"""The reference's behaviour-cloning loop restated in torch on the CPU (the comparator of
test_gpu_bcfit.py and tools/bcfit_time.py): BC.fit (mjrl/mjrl/algos/behavior_cloning.py:106-139)
over the policy's tanh MLP with flat-order parameters (gaussian_mlp.py:36-41),
torch.optim.Adam, nn.MSELoss or -mean(LL) (gaussian_mlp.py:117-121) and injected index
batches.  It runs in fp64 (the yardstick) or fp32 (the reference's own arithmetic: at the
inputs below it is bit-identical to the reference's BC.train)."""
import numpy as np
import torch
import torch.nn.functional as F

HIDDEN = (32, 32)


def make_paths(lens, S, A, seed=5):
    """Seeded expert paths: act = tanh(obs Wt) + noise, float64 like the reference's paths."""
    rs = np.random.RandomState(seed)
    Wt = rs.randn(S, A) * 0.05
    paths = []
    for l in lens:
        obs = rs.randn(l, S)
        act = np.tanh(obs @ Wt) + 0.1 * rs.randn(l, A)
        paths.append(dict(observations=obs, actions=act))
    return paths


def concat(paths):
    return (np.concatenate([p["observations"] for p in paths]), np.concatenate([p["actions"] for p in paths]))


def param_shapes(S, A):
    return [(HIDDEN[0], S), (HIDDEN[0],), (HIDDEN[1], HIDDEN[0]), (HIDDEN[1],), (A, HIDDEN[1]), (A,), (A,)]


def split_flat(flat, S, A):
    out, o = [], 0
    for shape in param_shapes(S, A):
        n = int(np.prod(shape))
        out.append(np.asarray(flat[o:o + n]).reshape(shape))
        o += n
    assert o == len(flat)
    return out


class Host:
    """The reference policy's trainable_params (W1, b1, W2, b2, W3, b3, log_std) as leaf tensors
    of `dtype`, their torch.optim.Adam and BC's two losses."""

    def __init__(self, flat, S, A, dtype, loss_type="MSE", lr=1e-3):
        self.S, self.A, self.dtype, self.loss_type = S, A, dtype, loss_type
        self.params = [torch.tensor(np.asarray(p, dtype=np.float32)).to(dtype).requires_grad_(True)
                       for p in split_flat(flat, S, A)]
        self.optimizer = torch.optim.Adam(self.params, lr=lr)
        self.mse = torch.nn.MSELoss()

    def mean(self, x):
        W1, b1, W2, b2, W3, b3, _ = self.params
        return F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, W1, b1)), W2, b2)), W3, b3)

    def loss(self, x, a):
        mu = self.mean(x)
        if self.loss_type == "MSE":
            return self.mse(mu, a)
        log_std = self.params[-1]
        zs = (a - mu) / torch.exp(log_std)
        LL = - 0.5 * torch.sum(zs ** 2, dim=1) + - torch.sum(log_std) + - 0.5 * self.A * np.log(2 * np.pi)
        return -torch.mean(LL)

    def data(self, obs, act):
        """torch.from_numpy(x).float() (behavior_cloning.py:101-102), then this host's dtype."""
        return (torch.from_numpy(np.asarray(obs)).float().to(self.dtype),
                torch.from_numpy(np.asarray(act)).float().to(self.dtype))

    def fit(self, obs, act, batches):
        """BC.fit with `batches` [epochs][steps][64] in place of np.random.choice:
        (loss_before, [total loss per epoch], loss_after, [every step's loss])."""
        x, a = self.data(obs, act)
        with torch.no_grad():
            before = self.loss(x, a).item()
        totals, step_losses = [], []
        for epoch in batches:
            total = 0
            for idx in epoch:
                i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
                self.optimizer.zero_grad()
                loss = self.loss(x[i], a[i])
                total += loss.item()
                step_losses.append(loss.item())
                loss.backward()
                self.optimizer.step()
            totals.append(total)
        with torch.no_grad():
            after = self.loss(x, a).item()
        return before, totals, after, step_losses

    def flat(self):
        return np.concatenate([p.detach().numpy().ravel() for p in self.params])

    def adam(self):
        """(step, [exp_avg], [exp_avg_sq]) over the parameters that have state (six under MSE)."""
        st = [self.optimizer.state[p] for p in self.params if p in self.optimizer.state]
        if not st:
            return 0, [], []
        return int(st[0]["step"]), [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st]
