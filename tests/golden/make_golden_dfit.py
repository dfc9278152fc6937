"""Generate tests/golden/g16_disc_update.npz by running the REFERENCE's own GAILCost.update_disc /
compute_chi2_distance (milo/milo/gail_cost.py:94-228) on its AgentReplayBuffer
(milo/milo/datasets.py:51-104).

Dev-container only; reuses make_golden.py's stubs and exits cleanly without the reference.
The fixture holds results only: the inputs are regenerated from seeds by the tests
(tests/dfit_ref.py: G16, g16_inputs, g16_mb).  Two blocks of three update_disc calls each, then
compute_chi2_distance:
  sgd_ls   SGD with the reference defaults (lr 1e-5, momentum 0.9), least squares, bs 70 passed in
  adam_ll  Adam at lr 1e-3, log-likelihood, mb_ss=None (256 rows sampled from the buffer)
Recorded per block: the integers drawn from numpy's global generator, the per-step metrics, the
final weights, the optimizer state and the chi^2 value.

The generator also measures, per block and tensor, the distance between the reference's fp32 run
and the fp64 restatement (tests/dfit_ref.py) in the tests' metric, max |dW - dW_ref| / max |dW_ref|
of the update dW = W - W_init (and max |s - s_ref| / max |s_ref| of the optimizer state), prints
them and derives the tests' tolerances: 4 x the largest, rounded up to one significant digit.  It
asserts that the fp32 restatement, too, stays within a quarter of them of the reference (a ReLU
mask that flips between fp32 and fp64 moves the penalty's gradient discontinuously: choose other
seeds then).

Usage:  python tests/golden/make_golden_dfit.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import dfit_ref as R  # noqa: E402


def round_up_1sig(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def run_block(name, cfg):
    from milo.datasets import AgentReplayBuffer
    from milo.gail_cost import GAILCost
    G = R.G16
    expert, adds, agent = R.g16_inputs()
    rb = AgentReplayBuffer(max_size=G["max_size"])
    for s, s2 in adds:
        rb.add(s, s2)
    assert torch.equal(torch.cat([rb.states, rb.next_states], -1), agent)
    gc = GAILCost(expert, agent_rb=rb, hidden_dims=list(G["hidden"]), seed=cfg["seed"], disc_loss_type=cfg["loss"],
                  disc_opt=cfg["opt"], disc_opt_args=dict(cfg["args"]))
    params = list(gc.disc.parameters())
    init = [p.detach().clone() for p in params]
    draws, real = [], np.random.randint

    def logged(*a, **k):
        v = real(*a, **k)
        draws.append(np.asarray(v).copy())
        return v

    np.random.randint = logged
    try:
        mets = [gc.update_disc(R.g16_mb(cfg, k)) for k in range(G["steps"])]
        n_step_draws = len(draws)
        st = np.random.get_state()
        rng_after = np.concatenate([st[1], [st[2]]]).astype(np.int64)   # MT19937 key and position after the steps
        chi2 = gc.compute_chi2_distance()
    finally:
        np.random.randint = real
    per = n_step_draws // G["steps"]          # 1 draw per step (expert) or 2 (buffer, then expert)
    assert per == (1 if cfg["mb_seeds"] else 2) and len(draws) == n_step_draws + 1
    idx_e = np.stack([draws[k * per + per - 1] for k in range(G["steps"])])
    idx_m = np.stack([draws[k * per] for k in range(G["steps"])]) if per == 2 else None
    out = {f"{name}_idx_e": idx_e, f"{name}_chi2_idx": draws[-1], f"{name}_chi2": np.float64(chi2),
           f"{name}_rng_after": rng_after,
           f"{name}_metrics": np.array([[m[k] for k in R.METRICS] for m in mets], dtype=np.float64)}
    if idx_m is not None:
        out[f"{name}_idx_m"] = idx_m
    if cfg["loss"] == "least_squares":
        out[f"{name}_acc"] = np.array([[float(m["expert_acc"]), float(m["mb_acc"])] for m in mets])
    for j, p in enumerate(params):
        out[f"{name}_p{j}"] = p.detach().numpy().copy()
        st = gc.disc_opt.state[p]
        if cfg["opt"] == "sgd":
            out[f"{name}_p{j}_buf"] = st["momentum_buffer"].numpy().copy()
        else:
            out[f"{name}_p{j}_exp_avg"] = st["exp_avg"].numpy().copy()
            out[f"{name}_p{j}_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
            out[f"{name}_step"] = np.float64(float(st["step"]))

    # distances to the restatement, fp64 and fp32
    batches = [(expert[idx_e[k]], R.g16_mb(cfg, k) if idx_m is None else agent[idx_m[k]]) for k in range(G["steps"])]
    p1 = cfg["args"].get("momentum", 1e-8)
    dist = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        r = R.restate(init, batches, cfg["loss"], cfg["opt"], cfg["args"]["lr"], p1, 0.5, 0.05, 10.0, dt)
        dw = [R.update_error(params[j].detach(), r["weights"][j], init[j]) for j in range(6)]
        ds = [R.state_error(out[f"{name}_p{j}_" + ("buf" if cfg["opt"] == "sgd" else "exp_avg")], r["state"]["s1"][j])
              for j in range(6)]
        if cfg["opt"] != "sgd":
            ds += [R.state_error(out[f"{name}_p{j}_exp_avg_sq"], r["state"]["s2"][j]) for j in range(6)]
        dm = max(abs(mets[k][key] - r["metrics"][k][key]) / abs(r["metrics"][k][key])
                 for k in range(G["steps"]) for key in R.METRICS)
        dist[tag] = (max(dw), max(ds), dm)
        print(f"[make_golden_dfit] {name}: reference fp32 vs restatement {tag}: dW {max(dw):.3e} "
              f"(per tensor {', '.join(f'{v:.1e}' for v in dw)}), state {max(ds):.3e}, metrics {dm:.3e}")
    x_chi = expert[draws[-1]]
    c64 = R.chi2([p.detach() for p in params], x_chi, agent, 0.5, torch.float64)
    print(f"[make_golden_dfit] {name}: chi2 {chi2!r} vs fp64 restatement {c64!r}")
    assert abs(chi2 - c64) <= 2.5e-5 * abs(c64)
    out[f"{name}_dist"] = np.array(dist["f64"][:2])
    return out, dist


def main():
    if not os.path.isdir(os.path.join(MG.REF, "milo")):
        print(f"[make_golden_dfit] {MG.REF} not present: nothing to do")
        return 0
    MG.install_stubs()
    torch.set_num_threads(1)
    out, dists = {}, {}
    for name, cfg in R.G16["blocks"].items():
        o, d = run_block(name, cfg)
        out.update(o)
        dists[name] = d
    tol_dw = round_up_1sig(4 * max(d["f64"][0] for d in dists.values()))
    tol_state = round_up_1sig(4 * max(d["f64"][1] for d in dists.values()))
    print(f"[make_golden_dfit] TOL_DW = {tol_dw:g}, TOL_STATE = {tol_state:g}")
    for name, d in dists.items():
        assert d["f64"][0] <= tol_dw / 4 and d["f64"][1] <= tol_state / 4, (name, d)
        assert d["f32"][0] <= tol_dw / 4 and d["f32"][1] <= tol_state / 4, \
            f"{name}: the fp32 restatement is {d['f32']} from the reference (a flipped ReLU mask?): choose other seeds"
        assert d["f64"][2] <= 2.5e-5 and d["f32"][2] <= 2.5e-5, (name, d)
    out["tol_dw"], out["tol_state"] = np.float64(tol_dw), np.float64(tol_state)
    assert all(np.isfinite(v).all() for v in out.values() if isinstance(v, np.ndarray) and v.dtype.kind == "f")
    path = os.path.join(HERE, "g16_disc_update.npz")
    np.savez_compressed(path, **out)
    print("[make_golden_dfit] wrote", path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
