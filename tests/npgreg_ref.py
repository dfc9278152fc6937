"""Host comparator of the NPG update as run.py builds it (mjrl/mjrl/algos/npg_cg.py:68-199 with
bc_args and hvp_sample_frac < 1), built from oracle.milo_ref's npg_vpg, npg_hvp and cg_solve:

  * VPG = the rollout's VPG + npg_vpg(expert rows, adv == reg_coeff): at new == old the gradient
    of reg_coeff * mean(LL) is the likelihood-ratio gradient with constant advantages;
  * the Fisher-vector product of CG iteration i is npg_hvp on obs[idx_i], idx_i the i-th
    np.random.choice(N, size=int(frac * N)) of the stream (NPG.HVP draws once per product).

`update` is the fp32 form (torch-CPU float32 autograd, as the reference); `update64` restates
it in float64 on the same draws: the yardstick of the tests' bounds.  No reference import.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import milo_ref as R

STEP, DAMPING, CG_ITERS, MIN_LOG_STD = 0.1, 1e-4, 10, -2.0
# the project's bounds for the NPG update (tests/test_gpu_npg.py; surr_before: tests/test_gpu_ppo.py)
TOL_VPG, TOL_NPG, RTOL_SURR, ATOL_SURR_BEFORE = 1e-4, 2e-3, 1e-3, 1e-6

# the three conditioned shapes of test_npg_vs_oracle_rollout_size
SHAPES = [(197, 36, 4096), (226, 28, 1000), (111, 8, 2048)]
FRACS = [0.5, 0.3]
N_EXPERT, REG_COEFF, EXPERT_SHIFT, DRAW_SEED = 256, 0.05, 0.25, 23
CASES = [(S, A, n, frac, bc) for (S, A, n) in SHAPES for frac in FRACS for bc in (False, True)]


def maxrel(x, ref) -> float:
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def draws(seed, n: int, frac: float, iters: int = CG_ITERS):
    """The index vectors NPG.HVP draws in one solve, from a generator seeded with `seed` (the
    legacy stream np.random.seed(seed) starts) or from a given RandomState."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    return [rs.choice(n, size=int(frac * n)) for _ in range(iters)]


def policy_mean(flat, S, A, obs):
    h = torch.from_numpy(np.asarray(obs)).float()
    p = R._unflatten(flat, R.policy_param_shapes(S, A))
    for j in range(3):
        h = F.linear(h, p[2 * j], p[2 * j + 1])
        h = torch.tanh(h) if j < 2 else h
    return h.numpy()


def expert_rows(flat, S, A, n=N_EXPERT, seed=29, shift=EXPERT_SHIFT):
    """A synthetic expert: float32-representable observations, actions around the policy mean
    moved by `shift` (a systematic pull: the BC gradient does not average out)."""
    rs = np.random.RandomState(seed)
    obs = (0.5 * rs.randn(n, S)).astype(np.float32).astype(np.float64)
    act = policy_mean(flat, S, A, obs).astype(np.float64) + shift + 0.5 * np.exp(-0.25) * rs.randn(n, A)
    return obs, act


@functools.lru_cache(maxsize=None)
def case_inputs(S, A, n):
    """test_npg_vs_oracle_rollout_size's inputs at one shape, plus an expert set."""
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    layers, ls = init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25)
    p0 = pack_policy(layers, ls)
    rs = np.random.RandomState(7)
    obs = (0.5 * rs.randn(n, S)).astype(np.float32).astype(np.float64)
    act = policy_mean(p0, S, A, obs).astype(np.float64) + np.exp(-0.25) * rs.randn(n, A)
    adv = rs.randn(n) * 1.5 + 0.2
    adv_w = (adv - np.mean(adv)) / (np.std(adv) + 1e-6)
    eo, ea = expert_rows(p0, S, A)
    return dict(p0=p0, obs=obs, act=act, adv=adv, adv_w=adv_w, expert_obs=eo, expert_act=ea)


# ---- fp32: oracle.milo_ref ---------------------------------------------------------------------

def _ll32(flat, shapes, obs, act):
    A = shapes[-1][0]
    o, a = torch.from_numpy(np.asarray(obs)).float(), torch.from_numpy(np.asarray(act)).float()
    return R._policy_mean_ll(R._unflatten(flat, shapes), o, a, A)[1]


def update(flat, S, A, obs, act, adv_w, idx=None, bc=None, step=STEP, damping=DAMPING, cg_iters=CG_ITERS,
           min_log_std=MIN_LOG_STD, residual_tol=1e-10):
    """One NPG.train_from_paths on whitened advantages.  idx: the solve's index vectors (None:
    the full Fisher); bc: (expert_obs, expert_act, reg_coeff) or None."""
    shapes = R.policy_param_shapes(S, A)
    flat = np.asarray(flat, dtype=np.float32)
    vpg_roll, surr0 = R.npg_vpg(flat, shapes, obs, act, adv_w)
    vpg, vpg_bc, surr_before = vpg_roll, None, np.float32(surr0)
    if bc is not None:
        eo, ea, reg = bc
        vpg_bc, _ = R.npg_vpg(flat, shapes, eo, ea, np.full(len(eo), reg))
        vpg = vpg_roll + vpg_bc
        surr_before = np.float32(surr_before + np.float32(reg) * _ll32(flat, shapes, eo, ea).mean().numpy())
    taken = [0]

    def f_Ax(v):
        rows = slice(None) if idx is None else idx[taken[0]]
        taken[0] += 1
        return R.npg_hvp(flat, shapes, obs[rows], act[rows], v, damping)

    npg = R.cg_solve(f_Ax, vpg, cg_iters=cg_iters, residual_tol=residual_tol)
    alpha = np.sqrt(np.abs(step / (np.dot(vpg.T, npg) + 1e-20)))
    new32 = np.asarray(flat + alpha * npg).astype(np.float32)
    new32[-A:] = np.maximum(new32[-A:], np.float32(min_log_std))
    sa, _ = R._cpi_surrogate(new32, flat, shapes, obs, act, adv_w)
    surr_after = np.float32(sa.data.numpy())
    if bc is not None:
        surr_after = np.float32(surr_after + np.float32(bc[2]) * _ll32(new32, shapes, bc[0], bc[1]).mean().numpy())
    ll_old, ll_new = _ll32(flat, shapes, obs, act).numpy(), _ll32(new32, shapes, obs, act).numpy()
    return dict(vpg=vpg, vpg_rollout=vpg_roll, vpg_bc=vpg_bc, npg=npg, alpha=float(alpha), params1=new32,
                surr_before=float(surr_before), surr_after=float(surr_after), products=taken[0], ll_old=ll_old,
                ll_new=ll_new)


# ---- fp64 restatement ----------------------------------------------------------------------------

def _unflat64(flat, shapes, grad=False):
    out, i = [], 0
    for sh in shapes:
        k = int(np.prod(sh))
        out.append(torch.from_numpy(np.asarray(flat[i:i + k], dtype=np.float64).reshape(sh).copy()).requires_grad_(grad))
        i += k
    return out


def _surr64(new, old, obs, act, adv, A, bc):
    _, ll_old = R._policy_mean_ll(old, obs, act, A)
    _, ll_new = R._policy_mean_ll(new, obs, act, A)
    surr = torch.mean(torch.exp(ll_new - ll_old) * adv)
    if bc is not None:
        surr = surr + bc[2] * torch.mean(R._policy_mean_ll(new, bc[0], bc[1], A)[1])
    return surr


def update64(flat, S, A, obs, act, adv_w, idx=None, bc=None, step=STEP, damping=DAMPING, cg_iters=CG_ITERS,
             min_log_std=MIN_LOG_STD, residual_tol=1e-10):
    """`update` in float64 from the same float32 parameters and rows, on the same draws."""
    shapes = R.policy_param_shapes(S, A)
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    flat = np.asarray(flat, dtype=np.float32).astype(np.float64)
    o, a, adv = t(np.asarray(obs, np.float32)), t(np.asarray(act, np.float32)), t(adv_w)
    bct = None if bc is None else (t(np.asarray(bc[0], np.float32)), t(np.asarray(bc[1], np.float32)), float(bc[2]))
    old = _unflat64(flat, shapes)

    def grad(bc_):
        new = _unflat64(flat, shapes, grad=True)
        surr = _surr64(new, old, o, a, adv, A, bc_)
        g = torch.autograd.grad(surr, new)
        return np.concatenate([x.reshape(-1).numpy() for x in g]), float(surr.detach())

    vpg, surr_before = grad(bct)
    taken = [0]

    def f_Ax(v):
        rows = slice(None) if idx is None else torch.from_numpy(np.asarray(idx[taken[0]]))
        taken[0] += 1
        new = _unflat64(flat, shapes, grad=True)
        om, _ = R._policy_mean_ll(old, o[rows], a[rows], A)
        nm, _ = R._policy_mean_ll(new, o[rows], a[rows], A)
        g = torch.autograd.grad(R._mean_kl(nm, new[-1], om, old[-1]), new, create_graph=True)
        h = torch.sum(torch.cat([x.reshape(-1) for x in g]) * t(v))
        hv = torch.autograd.grad(h, new)
        return np.concatenate([x.reshape(-1).numpy() for x in hv]) + damping * np.asarray(v, np.float64)

    npg = R.cg_solve(f_Ax, vpg, cg_iters=cg_iters, residual_tol=residual_tol)
    alpha = np.sqrt(np.abs(step / (np.dot(vpg, npg) + 1e-20)))
    new32 = (flat + alpha * npg).astype(np.float32)
    new32[-A:] = np.maximum(new32[-A:], np.float32(min_log_std))
    with torch.no_grad():
        surr_after = float(_surr64(_unflat64(new32, shapes), old, o, a, adv, A, bct))
    return dict(vpg=vpg, npg=npg, alpha=float(alpha), params1=new32, params1_64=flat + alpha * npg,
                surr_before=surr_before, surr_after=surr_after, products=taken[0])


@functools.lru_cache(maxsize=None)
def case_ref(S, A, n, frac, with_bc, seed=DRAW_SEED, f64=False):
    """The comparator's update of one case (computed once per process)."""
    c = case_inputs(S, A, n)
    bc = (c["expert_obs"], c["expert_act"], REG_COEFF) if with_bc else None
    idx = None if frac is None else draws(seed, n, frac)
    fn = update64 if f64 else update
    out = fn(c["p0"], S, A, c["obs"], c["act"], c["adv_w"], idx=idx, bc=bc)
    out["idx"] = idx
    return out
