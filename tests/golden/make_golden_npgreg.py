"""Generate tests/golden/g23_npg_reg.npz by running the REFERENCE's own NPG
(mjrl/mjrl/algos/npg_cg.py:25-199) as run.py builds it: hvp_sample_frac = 0.5 and bc_args with a
synthetic expert path, two consecutive train_from_paths calls on one agent.

Dev-container only; reuses make_golden.py's REF, OUT and stubs and exits cleanly without the
reference.  The fixture holds recorded arrays and settings only.  Policy and settings are G11's
(MLP(32, 32), seed 100, init_log_std -0.25, min_log_std -2, normalized_step_size 0.1, 10 CG
iterations, damping 1e-4); the paths are g11_paths' recipe at the lengths below, drawn from the
policy as it stands before each call.  Recorded per call: the inputs, the index vectors (re-drawn
from the seed; the stream's end state is checked against the run's), vpg_grad, npg_grad, alpha,
surr_before, surr_after, kl_dist, running_score, the parameters after the call, old_dist_info[0],
new_dist_info[0] and lr; and numpy's generator state after the second call.

The generator also prints the conditions tests/test_cpu_npgreg.py asserts (the BC gradient's
size against the rollout's, what subsampling moves, the fp32 comparator's distance from its fp64
restatement): DESIGN.md quotes them.

Usage:  python tests/golden/make_golden_npgreg.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
import npgreg_ref as G  # noqa: E402

S, A = MG.S, MG.A
LENGTHS = (7, 1, 30, 12, 50, 3, 25, 64, 39)  # g11_paths' lengths and one more path: 231 rows
NUMPY_SEED, FRAC, N_EXPERT, REG_COEFF = 2300, 0.5, 96, 0.1
CONFIG = dict(step=0.1, damping=1e-4, cg_iters=10, min_log_std=-2.0, frac=FRAC, numpy_seed=NUMPY_SEED,
              reg_coeff=REG_COEFF, model_seed=100, init_log_std=-0.25)


def paths_for(pol, seed):
    rs = np.random.RandomState(seed)
    paths = []
    for T in LENGTHS:
        obs = (0.5 * rs.randn(T, S)).astype(np.float32).astype(np.float64)
        obs[:, 0] = rs.uniform(0.8, 0.95, T).astype(np.float32)
        mean = pol.model(torch.from_numpy(obs).float()).detach().numpy()
        act = mean.astype(np.float64) + np.exp(-0.25) * rs.randn(T, A)
        paths.append(dict(observations=obs, actions=act, advantages=rs.randn(T) * 2.0 + 0.3, rewards=rs.randn(T)))
    return paths


def main():
    if not os.path.isdir(os.path.join(MG.REF, "mjrl")):
        print(f"[make_golden_npgreg] {MG.REF} not present: nothing to do")
        return 0
    MG.install_stubs()
    torch.set_num_threads(1)
    from mjrl.algos.npg_cg import NPG
    from mjrl.policies.gaussian_mlp import MLP

    pol = MLP(S, A, hidden_sizes=(32, 32), seed=100, init_log_std=-0.25, min_log_std=-2.0)
    p0 = pol.get_param_values()
    eo, ea = G.expert_rows(p0, S, A, n=N_EXPERT)
    bc_args = {"flag": True, "expert_paths": {"observations": eo, "actions": ea}, "reg_coeff": REG_COEFF}
    agent = NPG(None, pol, None, normalized_step_size=0.1, FIM_invert_args={"iters": 10, "damping": 1e-4},
                hvp_sample_frac=FRAC, seed=100, save_logs=True, bc_args=bc_args)
    out = {k: np.asarray(v) for k, v in CONFIG.items()}
    out.update(params0=p0, expert_obs=eo.astype(np.float32), expert_act=ea, lengths=np.asarray(LENGTHS))
    redraw = np.random.RandomState(NUMPY_SEED)
    np.random.seed(NUMPY_SEED)
    params = p0
    for k in range(2):
        paths = paths_for(pol, seed=11 + k)
        infos = {}
        agent.train_from_paths(paths, infos)
        n = sum(LENGTHS)
        idx = np.asarray(G.draws(redraw, n, FRAC), dtype=np.int32)
        obs, act = (np.concatenate([p[key] for p in paths]) for key in ("observations", "actions"))
        rec = dict(observations=obs.astype(np.float32), actions=act,
                   advantages=np.concatenate([p["advantages"] for p in paths]),
                   rewards=np.concatenate([p["rewards"] for p in paths]), adv_whitened=infos["advantages"], idx=idx,
                   vpg=infos["vpg_grad"], npg=infos["npg_grad"], alpha=np.float64(infos["alpha"]),
                   surr_before=np.float64(infos["surr_before"]), surr_after=np.float64(infos["surr_after"]),
                   kl_dist=np.float64(infos["kl_dist"]), running_score=np.float64(infos["running_score"]),
                   params=pol.get_param_values(), ll_old=infos["old_dist_info"][0].data.numpy(),
                   ll_new=infos["new_dist_info"][0].data.numpy(), lr=infos["lr"].data.numpy())
        out.update({f"c{k}__{key}": v for key, v in rec.items()})
        # the conditions of the tests, on the comparator
        bc = (eo, ea, REG_COEFF)
        adv_w = infos["advantages"]
        r32 = G.update(params, S, A, obs, act, adv_w, idx=list(idx), bc=bc)
        r64 = G.update64(params, S, A, obs, act, adv_w, idx=list(idx), bc=bc)
        full = G.update(params, S, A, obs, act, adv_w, idx=None, bc=bc)
        other = G.update(params, S, A, obs, act, adv_w, idx=G.draws(NUMPY_SEED + 1 + k, n, FRAC), bc=bc)
        dp = lambda r: np.asarray(r["params1"], np.float64) - params
        print(f"[call {k}] products {r32['products']}  |bc grad| / |rollout vpg| "
              f"{np.linalg.norm(r32['vpg_bc']) / np.linalg.norm(r32['vpg_rollout']):.3f}\n"
              f"  comparator vs reference: vpg {G.maxrel(r32['vpg'], rec['vpg']):.2e} npg {G.maxrel(r32['npg'], rec['npg']):.2e}"
              f" dparams {G.maxrel(dp(r32), rec['params'] - params):.2e}"
              f" surr_after rel {abs(r32['surr_after'] / rec['surr_after'] - 1):.2e}"
              f" surr_before abs {abs(r32['surr_before'] - rec['surr_before']):.2e}\n"
              f"  subsampled vs full Fisher npg {G.maxrel(full['npg'], r32['npg']):.3f}; vs another seed's draws "
              f"{G.maxrel(other['npg'], r32['npg']):.3f}\n"
              f"  fp32 vs fp64 comparator: vpg {G.maxrel(r32['vpg'], r64['vpg']):.2e} npg {G.maxrel(r32['npg'], r64['npg']):.2e}"
              f" dparams {G.maxrel(dp(r32), r64['params1_64'] - params):.2e}"
              f" surr_after rel {abs(r32['surr_after'] / r64['surr_after'] - 1):.2e}"
              f" surr_before abs {abs(r32['surr_before'] - r64['surr_before']):.2e}")
        params = pol.get_param_values()
    st, end = np.random.get_state(), redraw.get_state()
    assert st[2] == end[2] and np.array_equal(st[1], end[1]), "the re-drawn index vectors are not the run's"
    out.update(rng_keys=st[1], rng_pos=np.int64(st[2]), rng_has_gauss=np.int64(st[3]), rng_gauss=np.float64(st[4]))
    path = os.path.join(MG.OUT, "g23_npg_reg.npz")
    np.savez_compressed(path, **out)
    print("[make_golden_npgreg] wrote", path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
