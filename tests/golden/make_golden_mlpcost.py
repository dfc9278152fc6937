"""Generate tests/golden/g22_mlp_cost.npz by running the REFERENCE's own MLPCost
(milo/milo/linear_cost.py:154-301) and, for the disagreement bonus, its DynamicsEnsemble.

Dev-container only; reuses make_golden.py's REF, OUT and stubs and exits cleanly without the
reference.  The fixture holds recorded arrays and seeds only: the inputs are regenerated from the
seeds by the tests (tests/mlpcost_ref.py: G22, G22_COMMON, synthetic_rows).  Three variants:
  deep  'ss', S 24, hidden_dims [64, 96, 64], F 128, cost_range [-1, 0]
  flat  'ss', hidden_dims [] (the net is Linear(D, F), Tanh), F 256, cost_range None
  sa    'sa', A 6, hidden_dims [128, 128], F 128
each with 300 expert rows, 200 policy rows (shifted by +0.3 so that w != 0) and lambda_b 0.1.
Recorded per variant: net.state_dict(), bw, phi_e, phi of every fourth policy row (the fixture
stays small; every row enters w), w, mb_mmd, get_costs,
get_bonus_costs with its info dict, and get_expert_cost where a cost range exists.  The ensemble
follows G5: the reference's 4 x [64]*4 dense-connect ensemble at base_seed 100 on 2048 synthetic
offline rows, its threshold recorded.

The generator also prints, per variant, the reference's fp32 distance from the fp64 restatement
(tests/mlpcost_ref.py) -- the yardstick of the tests' bounds.

Usage:  python tests/golden/make_golden_mlpcost.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import mlpcost_ref as R  # noqa: E402


def main():
    if not os.path.isdir(os.path.join(MG.REF, "milo")):
        print(f"[make_golden_mlpcost] {MG.REF} not present: nothing to do")
        return 0
    MG.install_stubs()
    torch.set_num_threads(1)
    from milo.datasets import AmpDataset
    from milo.dynamics import DynamicsEnsemble
    from milo.linear_cost import MLPCost

    C = R.G22_COMMON
    out = {k: np.asarray(v) for k, v in C.items()}
    for name, cfg in R.G22.items():
        S, A = cfg["S"], cfg["A"]
        ds = AmpDataset(*R.synthetic_rows(C["n_offline"], C["offline_seed"], S, A))
        ens = DynamicsEnsemble(S, A, ds, None, num_models=4, hidden_sizes=list(C["ens_hidden"]), dense_connect=True,
                               transform=True, base_seed=C["ens_seed"])
        for m in ens.models:  # as load_ensemble does (dynamics.py:128-131)
            m.state_mean, m.state_scale, m.action_mean, m.action_scale, m.diff_mean, m.diff_scale = ens.transformations
        ens.compute_threshold()
        es, ea, es2 = R.synthetic_rows(C["n_expert"], C["expert_seed"], S, A)
        ps, pa, ps2 = R.synthetic_rows(C["n_pi"], C["pi_seed"], S, A, shift=C["pi_shift"])
        expert, x_pi = R.cost_rows(cfg["input_type"], es, ea, es2), R.cost_rows(cfg["input_type"], ps, pa, ps2)
        cost = MLPCost(expert, hidden_dims=list(cfg["hidden_dims"]), activation="relu", feature_dim=cfg["feature_dim"],
                       input_type=cfg["input_type"], cost_range=cfg["cost_range"], bw_quantile=C["bw_quantile"],
                       bw_samples=C["bw_samples"], lambda_b=C["lambda_b"], seed=C["seed"])
        mb_mmd = cost.fit_cost(x_pi)
        phi_pi = cost.get_rep(x_pi)
        costs = cost.get_costs(x_pi)
        bc, info = cost.get_bonus_costs(ps, pa, ens, next_states=ps2)
        rec = dict(bw=np.float64(cost.bw), phi_e=cost.phi_e.numpy(), phi_pi=phi_pi.numpy()[::R.G22_PHI_STRIDE],
                   w=cost.w.numpy(),
                   mb_mmd=np.float64(mb_mmd), costs=costs.numpy(), threshold=np.float64(ens.threshold),
                   cost=bc.numpy(), ipm=info["ipm"].numpy(), bonus=info["bonus"].numpy(),
                   v_targ=info["v_targ"].numpy())
        if cfg["cost_range"] is not None:
            rec["expert_cost"] = np.float64(cost.get_expert_cost().item())
        sd = {k: v.numpy() for k, v in cost.net.state_dict().items()}
        out.update({f"{name}__{k}": v for k, v in rec.items()})
        out.update({f"{name}__sd__{k}": v for k, v in sd.items()})
        ref = R.Ref64(sd, expert, cfg["feature_dim"], cfg["cost_range"], C["lambda_b"])
        mmd64 = ref.fit_cost(x_pi)
        y = R.Yardstick(ref, expert, x_pi)
        print(f"[{name}] phi in [{ref.expert_rep.min():.5f}, {ref.expert_rep.max():.5f}]  max|w| {np.abs(ref.w).max():.3e}"
              f"  fp32 error: phi {np.abs(rec['phi_pi'] - ref.rep(x_pi)[::R.G22_PHI_STRIDE]).max():.2e} (here {y.phi_err:.2e})"
              f"  w {np.abs(rec['w'] - ref.w).max():.2e} = {np.abs(rec['w'] - ref.w).max() / np.abs(ref.w).max():.1e} of |w|"
              f" (here {y.w_err:.2e})  mb_mmd rel {abs(mb_mmd - mmd64) / mmd64:.1e}")
    path = os.path.join(MG.OUT, "g22_mlp_cost.npz")
    np.savez_compressed(path, **out)
    print("[make_golden_mlpcost] wrote", path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
