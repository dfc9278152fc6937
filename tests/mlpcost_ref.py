"""MLPCost (milo/milo/linear_cost.py:154-301) restated in fp64, its fp32 yardstick, the seeded
synthetic rows of the MLPCost tests and the error bounds they share.

The project's usual "1e-4 relative" gate does not fit this cost: a default-initialised net barely
moves phi (0.0622-0.0625 at F 512), so w = mean phi_pi - mean phi_e is a difference of nearly
equal means (max |w| 3e-5) and the reference's own fp32 run is 4e-4 of |w| away from an fp64 copy
of its net.  So every device result is compared with the fp64 restatement on the same weights,
and the measure of "close enough" is the error of the torch-CPU fp32 evaluation of the same net
-- exactly what the reference computes -- on the test's own rows:

  phi, per element          |phi_dev - phi_64| <= 4 x max |phi_32 - phi_64|
                            (the yardstick is its final rounding, ~0.6 ulp; another summation
                            order and <= 1-ulp tanh and cos land within ~2 ulp)
  w and phi_e, per element  <= 2 x the yardstick's error (fp64 sums: only per-element errors remain)
  phi . w                   ||phi||_1 dw + ||w||_1 dphi + 4 ulp of the value
  w . w                     2 ||w||_1 dw + 4 ulp of the value
  clamp, (1 - lambda) x, the bonus term, means: 1-Lipschitz / linear in the above, + 4 ulp of
                            the largest term (each is a handful of fp32 roundings)

A scalar is never measured on itself: one number's fp32 error can be near zero by accident.
"""
from __future__ import annotations

import numpy as np
import torch

# the variants of tests/golden/g22_mlp_cost.npz (make_golden_mlpcost.py).  `deep` hits a K tail
# (D 48 -> 64), a padded width (96 -> 128) and a row count that is no multiple of 128 (200 -> 256:
# n_valid and the row mask)
G22 = {
    "deep": dict(input_type="ss", S=24, A=6, hidden_dims=[64, 96, 64], feature_dim=128, cost_range=[-1.0, 0.0]),
    "flat": dict(input_type="ss", S=24, A=6, hidden_dims=[], feature_dim=256, cost_range=None),
    "sa": dict(input_type="sa", S=24, A=6, hidden_dims=[128, 128], feature_dim=128, cost_range=[-1.0, 0.0]),
}
G22_COMMON = dict(n_expert=300, n_pi=200, lambda_b=0.1, seed=100, bw_quantile=0.1, bw_samples=100000,
                  expert_seed=3, pi_seed=4, offline_seed=0, n_offline=2048, ens_hidden=[64] * 4, ens_seed=100,
                  pi_shift=0.3)
G22_PHI_STRIDE = 4   # the fixture records phi of policy rows 0, 4, 8, ...


def synthetic_rows(n: int, seed: int, S: int, A: int, shift: float = 0.0):
    """(s, a, s') float32 tensors: s ~ 0.5 N(0,1) with column 0 ~ U(0.8, 0.95), a ~ N(0,1),
    s' = s + 0.01 N(0,1); `shift` is added to s and s' (the policy rows: w != 0)."""
    rs = np.random.RandomState(seed)
    s = 0.5 * rs.randn(n, S)
    s[:, 0] = rs.uniform(0.8, 0.95, n)
    a = rs.randn(n, A)
    s2 = s + 0.01 * rs.randn(n, S)
    return tuple(torch.from_numpy(x).float() for x in (s + shift, a, s2 + shift))


def cost_rows(input_type: str, s, a, s2) -> torch.Tensor:
    return {"ss": lambda: torch.cat([s, s2], 1), "sa": lambda: torch.cat([s, a], 1),
            "sas": lambda: torch.cat([s, a, s2], 1), "s": lambda: s}[input_type]()


def linears(sd) -> list:
    """[(W, b), ...] of a net state_dict ('0.weight', '2.weight', ...) in layer order."""
    idx = sorted({int(k.split(".")[0]) for k in sd})
    return [(sd[f"{i}.weight"], sd[f"{i}.bias"]) for i in idx]


def phi64(sd, x, feature_dim: int) -> np.ndarray:
    """cos(tanh(net(x))) sqrt(2/F) in fp64 on the fp32 weights and rows."""
    h = np.asarray(x, np.float64)
    layers = linears(sd)
    for i, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if i + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return np.cos(np.tanh(h)) * np.sqrt(2 / feature_dim)


@torch.no_grad()
def phi32(sd, x, feature_dim: int) -> torch.Tensor:
    """The reference's get_rep: the same net in torch-CPU fp32, torch.cos(.) * np.sqrt(2/F)."""
    h = torch.as_tensor(x, dtype=torch.float32)
    layers = linears(sd)
    for i, (W, b) in enumerate(layers):
        h = torch.nn.functional.linear(h, torch.as_tensor(W), torch.as_tensor(b))
        if i + 1 < len(layers):
            h = torch.relu(h)
    return torch.cos(torch.tanh(h)) * np.sqrt(2 / feature_dim)


class Ref64:
    """The cost in fp64: phi_e, fit_cost, get_costs, the bonus cost given the disagreement,
    the expert cost."""

    def __init__(self, sd, expert, feature_dim, cost_range, lambda_b):
        self.sd, self.F, self.cost_range, self.lam = sd, feature_dim, cost_range, float(lambda_b)
        self.expert_rep = phi64(sd, expert, feature_dim)
        self.phi_e = self.expert_rep.mean(0)
        self.w = None

    def rep(self, x):
        return phi64(self.sd, x, self.F)

    def fit_cost(self, x) -> float:
        self.w = self.rep(x).mean(0) - self.phi_e
        return float(self.w @ self.w)

    def clamp(self, v):
        return v if self.cost_range is None else np.clip(v, self.cost_range[0], self.cost_range[1])

    def get_costs(self, x):
        return self.clamp(self.rep(x) @ self.w)

    def bonus_costs(self, x, disc, threshold):
        """(cost, ipm, weighted bonus) of linear_cost.py:261-301 from the disagreement `disc`."""
        c = self.get_costs(x)
        d = np.asarray(disc, np.float64)
        bonus = np.minimum(d / threshold, 1.0) * self.cost_range[0] if self.cost_range is not None else d
        ipm, wb = (1 - self.lam) * c, self.lam * bonus
        return ipm - wb, ipm, wb

    def expert_cost(self) -> float:
        return (1 - self.lam) * float(self.clamp(self.expert_rep @ self.w).mean())


class Yardstick:
    """The torch-CPU fp32 evaluation (what the reference computes) beside the fp64 restatement on
    the same rows: its errors are the unit of every bound."""

    def __init__(self, ref: Ref64, expert, x_pi):
        sd, F = ref.sd, ref.F
        pe32, pp32 = phi32(sd, expert, F), phi32(sd, x_pi, F)
        pp64 = ref.rep(x_pi)
        self.phi_err = max(np.abs(pe32.double().numpy() - ref.expert_rep).max(),
                           np.abs(pp32.double().numpy() - pp64).max())
        phi_e32 = pe32.mean(0)
        w32 = pp32.mean(0) - phi_e32
        w64 = pp64.mean(0) - ref.phi_e
        self.phi_e_err = np.abs(phi_e32.double().numpy() - ref.phi_e).max()
        self.w_err = np.abs(w32.double().numpy() - w64).max()
        self.phi32_pi, self.phi_e32, self.w32 = pp32, phi_e32, w32
        # the bounds of the module docstring
        self.d_phi, self.d_w, self.d_phi_e = 4 * self.phi_err, 2 * self.w_err, 2 * self.phi_e_err


def ulp4(*terms) -> float:
    """4 ulp (fp32) of the largest magnitude among `terms`."""
    m = max(float(np.abs(np.asarray(t, np.float64)).max()) for t in terms)
    return 4 * float(np.spacing(np.float32(m)))


def dot_bound(phi, w, d_phi: float, d_w: float) -> np.ndarray:
    """Per-row bound on phi . w: ||phi||_1 dw + ||w||_1 dphi + 4 ulp of the value."""
    phi, w = np.asarray(phi, np.float64), np.asarray(w, np.float64)
    v = np.abs(phi @ w)
    return np.abs(phi).sum(1) * d_w + np.abs(w).sum() * d_phi + 4 * np.spacing(v.astype(np.float32)).astype(np.float64)


def mmd_bound(w, d_w: float) -> float:
    """Bound on w . w: 2 ||w||_1 dw + 4 ulp of the value."""
    w = np.asarray(w, np.float64)
    return 2 * np.abs(w).sum() * d_w + ulp4(w @ w)
