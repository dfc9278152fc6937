"""Generate the G24 fixtures by running the REFERENCE's own plain (dense_connect=False)
DynamicsEnsemble (milo/milo/dynamics.py), at S/A = 197/36 with 4 members.

Dev-container only; reuses make_golden.py's stubs and exits cleanly without the reference.

  g24_plain_adam.pt, g24_plain_sgd.pt   the reference's save_ensemble files (a list of
        {'model', 'optim'}, dynamics.py:110-116) of a plain [32, 32] ensemble after one optimizer
        step per member on the offline set (amp_extensions_amd.synthetic.offline, 512 rows), with
        Adam at run.py's defaults and with SGD-Nesterov: what run.py without
        --dynamic_dense_connect writes.
  g24_plain.npz   of the Adam file loaded back as run.py:72-78 + 108 does: the threshold, every
        member's forward (un-normalised and normalised) and the disagreement on seeded query
        rows; of the reference's own BasicMLP / DynamicsModel.train_step in fp64 (member 0 of
        that file, the model cast with .double()): the forward on the query rows and, per
        optimizer, the loss and every parameter after one step of a fresh optimizer; and the
        scalars of the two training blocks below.
  g24_train_{adam,sgd}_{w,s1,s2}.npz   the reference's train(epochs=2, validate=True) on a plain
        [64, 64] ensemble, batch 64, 200 train rows (batches of 64, 64, 64, 8) and 100 validation
        rows (tests/efit_ref.py:synthetic_transitions), torch.manual_seed right before train:
        every member's final parameters (w), exp_avg or momentum_buffer (s1), exp_avg_sq (s2,
        Adam only), one file each to stay under the committed-file size limit.  The seed of a
        block is the first one from its start for which the fp32 reference stays within a
        quarter of test_gpu_efit.py's tolerances of the fp64 restatement (tests/plain_ref.py),
        the precondition those tolerances rest on.

Usage:  python tests/golden/make_golden_plain.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
import plain_ref as PR  # noqa: E402
from efit_ref import events_from_plan, synthetic_transitions  # noqa: E402

S, A, M = 197, 36, 4
CK_HIDDEN, N_OFFLINE, OFFLINE_SEED, BASE_SEED = [32, 32], 512, 24, 100
ADAM = {"optim": "adam", "lr": 1e-3, "eps": 1e-8}   # run.py's defaults (arguments.py:56-59)
SGD = {"optim": "sgd", "lr": 1e-4, "momentum": 0.9}  # DynamicsEnsemble's own default (dynamics.py:32)
TR_HIDDEN, BATCH, N_TRAIN, N_VAL, SEED_TRAIN, SEED_VAL, EPOCHS = [64, 64], 64, 200, 100, 241, 242, 2
BLOCKS = {
    "adam": dict(optim_args=ADAM, grad_clip=1.0, seed=2401),
    "sgd": dict(optim_args={"optim": "sgd", "lr": 0.05, "momentum": 0.9}, grad_clip=0.0, seed=2451),
}
TOL_W, TOL_LOSS, TOL_STATE = 2e-5, 1e-4, 1e-4  # test_gpu_efit.py's


def offline_tensors():
    from amp_extensions_amd.synthetic import offline
    return tuple(torch.from_numpy(x).float() for x in offline(N_OFFLINE, S, A, OFFLINE_SEED))


def set_transformations(ens):  # as DynamicsModel.train sets them (dynamics.py:311-313)
    for m in ens.models:
        m.state_mean, m.state_scale, m.action_mean, m.action_scale, m.diff_mean, m.diff_scale = ens.transformations


def make_checkpoints(out):
    from milo.datasets import AmpDataset
    from milo.dynamics import DynamicsEnsemble, DynamicsModel
    s, a, s2 = offline_tensors()
    ds = AmpDataset(s, a, s2)
    rs = np.random.RandomState(24)
    idx = rs.permutation(N_OFFLINE)[:64]
    qs = torch.from_numpy(rs.randn(48, S) * 0.5).float()
    qs[:, 0] = torch.from_numpy(rs.uniform(0.8, 0.95, 48)).float()
    qa = torch.from_numpy(rs.randn(48, A)).float()
    for name, oa in (("adam", ADAM), ("sgd", SGD)):
        kw = dict(num_models=M, batch_size=256, hidden_sizes=CK_HIDDEN, transform=True, dense_connect=False,
                  optim_args=oa, base_seed=BASE_SEED, device=torch.device("cpu"))
        ens = DynamicsEnsemble(S, A, ds, None, **kw)
        assert ens.models[0].model.dense_connect is False
        set_transformations(ens)
        for m in ens.models:
            m.train_step(0, ds.states[idx], ds.actions[idx], ds.next_states[idx])
        path = os.path.join(HERE, f"g24_plain_{name}.pt")
        ens.save_ensemble(path)
        print("[make_golden_plain] wrote", path, os.path.getsize(path), "bytes")
        if name != "adam":
            continue
        loaded = DynamicsEnsemble(S, A, ds, None, **kw)  # run.py:72-78 + 108 as written
        loaded.load_ensemble(path)
        loaded.compute_threshold()
        with torch.no_grad():
            out["preds"] = torch.stack([m.forward(qs, qa) for m in loaded.models]).numpy()
            out["preds_norm"] = torch.stack([m.forward(qs, qa, unnormalize_out=False) for m in loaded.models]).numpy()
        out["disc"] = loaded.get_action_discrepancy(qs, qa).numpy()
        out["threshold"] = np.float64(loaded.threshold)
        out["query_s"], out["query_a"], out["step_idx"] = qs.numpy(), qa.numpy(), idx
        # the reference's own BasicMLP and train_step in fp64: member 0's weights, fresh optimizers
        sd = copy.deepcopy(loaded.models[0].model.state_dict())
        tr64 = tuple(x.double() for x in loaded.transformations)
        for oname, ooa in (("adam", ADAM), ("sgd", BLOCKS["sgd"]["optim_args"])):
            dm = DynamicsModel(S, A, hidden_sizes=CK_HIDDEN, dense_connect=False, transform=True, optim_args=ooa,
                               device=torch.device("cpu"), seed=1)
            dm.model.load_state_dict(sd)
            dm.model.double()
            dm.state_mean, dm.state_scale, dm.action_mean, dm.action_scale, dm.diff_mean, dm.diff_scale = tr64
            if oname == "adam":
                with torch.no_grad():
                    out["f64_preds"] = dm.forward(qs.double(), qa.double()).numpy()
                    out["f64_raw"] = dm.model.forward(torch.cat([(qs.double() - tr64[0]) / tr64[1],
                                                                 (qa.double() - tr64[2]) / tr64[3]], 1)).numpy()
            out[f"f64_{oname}_loss"] = np.float64(dm.train_step(1.0, ds.states[idx].double(), ds.actions[idx].double(),
                                                                ds.next_states[idx].double()))
            for j, p in enumerate(dm.model.parameters()):
                assert p.dtype == torch.float64
                out[f"f64_{oname}_p{j}"] = p.detach().numpy().copy()


def restate(ens_sds, norms, tr, va, seed, oa, clip, dtype):
    from amp_extensions_amd.ensemble import index_loader, materialise, plan_batches
    torch.manual_seed(seed)
    plan, _ = plan_batches(N_TRAIN, N_VAL, BATCH, EPOCHS, M, True)
    tl, vl = index_loader(N_TRAIN, BATCH), index_loader(N_VAL, BATCH)
    p1 = oa["eps"] if oa["optim"] == "adam" else oa["momentum"]
    return [PR.restate_member(copy.deepcopy(sd), None, norms, {"train": tr, "val": va},
                              events_from_plan(plan[g], tl, vl, materialise), oa["optim"], oa["lr"], p1, clip, dtype)
            for g, sd in enumerate(ens_sds)]


def _rel_w(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def _rel_s(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300))


def run_block(name, cfg, seed):
    """The reference's train at `seed`: (fixture dict, worst fraction of a tolerance by which the
    fp32 reference run differs from the fp64 restatement)."""
    from milo.datasets import AmpDataset
    from milo.dynamics import DynamicsEnsemble
    tr, va = synthetic_transitions(N_TRAIN, S, A, SEED_TRAIN), synthetic_transitions(N_VAL, S, A, SEED_VAL)
    oa = cfg["optim_args"]
    ens = DynamicsEnsemble(S, A, AmpDataset(*tr), AmpDataset(*va), num_models=M, batch_size=BATCH,
                           hidden_sizes=TR_HIDDEN, transform=True, dense_connect=False, optim_args=oa,
                           base_seed=BASE_SEED, device=torch.device("cpu"))
    sds = [copy.deepcopy(m.model.state_dict()) for m in ens.models]
    r64 = restate(sds, ens.transformations, tr, va, seed, oa, cfg["grad_clip"], torch.float64)
    torch.manual_seed(seed)
    info = ens.train(EPOCHS, validate=True, grad_clip=cfg["grad_clip"])
    spe = -(-N_TRAIN // BATCH)
    scal = {f"{name}_info": np.array(info, dtype=np.float64), f"{name}_seed": seed,
            f"{name}_grad_clip": cfg["grad_clip"], f"{name}_lr": oa["lr"],
            f"{name}_p1": oa.get("eps", oa.get("momentum"))}
    files = {"w": {}, "s1": {}, "s2": {}}
    worst = 0.0
    for k, m in enumerate(ens.models):
        t64 = [l for kind, l in r64[k]["losses"] if kind == "t"]
        e64 = [float(np.average(t64[i:i + spe])) for i in range(0, len(t64), spe)]
        worst = max(worst, abs(info[k][0] - min(e64)) / abs(min(e64)) / TOL_LOSS,
                    abs(info[k][1] - e64[0]) / abs(e64[0]) / TOL_LOSS)
        names = list(m.model.state_dict())
        for j, p in enumerate(m.model.parameters()):
            files["w"][f"m{k}_p{j}"] = p.detach().numpy().copy()
            worst = max(worst, _rel_w(files["w"][f"m{k}_p{j}"], r64[k]["model"][names[j]].numpy()) / TOL_W)
            st, st64 = m.optimizer.state[p], r64[k]["optim"]["state"][j]
            if name == "adam":
                files["s1"][f"m{k}_p{j}"] = st["exp_avg"].numpy().copy()
                files["s2"][f"m{k}_p{j}"] = st["exp_avg_sq"].numpy().copy()
                scal[f"adam_m{k}_step"] = np.float64(float(st["step"]))
                worst = max(worst, _rel_s(st["exp_avg"].numpy(), st64["exp_avg"].numpy()) / TOL_STATE,
                            _rel_s(st["exp_avg_sq"].numpy(), st64["exp_avg_sq"].numpy()) / TOL_STATE)
            else:
                files["s1"][f"m{k}_p{j}"] = st["momentum_buffer"].numpy().copy()
                worst = max(worst, _rel_s(st["momentum_buffer"].numpy(), st64["momentum_buffer"].numpy()) / TOL_STATE)
    return scal, files, worst


def main():
    if not os.path.isdir(os.path.join(MG.REF, "milo")):
        print(f"[make_golden_plain] {MG.REF} not present: nothing to do")
        return 0
    MG.install_stubs()
    torch.set_num_threads(1)
    out = dict(S=S, A=A, M=M, ck_hidden=np.array(CK_HIDDEN), base_seed=BASE_SEED, n_offline=N_OFFLINE,
               offline_seed=OFFLINE_SEED, adam_lr0=ADAM["lr"], adam_eps0=ADAM["eps"], sgd_lr0=SGD["lr"],
               sgd_momentum0=SGD["momentum"], f64_sgd_lr=BLOCKS["sgd"]["optim_args"]["lr"],
               f64_sgd_momentum=BLOCKS["sgd"]["optim_args"]["momentum"], tr_hidden=np.array(TR_HIDDEN), batch=BATCH,
               n_train=N_TRAIN, n_val=N_VAL, seed_train=SEED_TRAIN, seed_val=SEED_VAL, epochs=EPOCHS)
    make_checkpoints(out)
    for name, cfg in BLOCKS.items():
        for seed in range(cfg["seed"], cfg["seed"] + 40):
            scal, files, worst = run_block(name, cfg, seed)
            print(f"[make_golden_plain] {name} seed {seed}: fp32 reference at {worst:.3f} of a tolerance from fp64")
            if worst <= 0.25:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps the fp32 reference within a quarter of the tolerances")
        out.update(scal)
        for kind, d in files.items():
            if d:
                path = os.path.join(HERE, f"g24_train_{name}_{kind}.npz")
                np.savez_compressed(path, **d)
                print("[make_golden_plain] wrote", path, os.path.getsize(path), "bytes")
                assert os.path.getsize(path) < 1 << 20
    assert all(np.isfinite(v).all() for v in out.values() if isinstance(v, np.ndarray))
    path = os.path.join(HERE, "g24_plain.npz")
    np.savez_compressed(path, **out)
    print("[make_golden_plain] wrote", path, os.path.getsize(path), "bytes")
    print("adam", out["adam_info"].tolist())
    print("sgd", out["sgd_info"].tolist())
    return 0


if __name__ == "__main__":
    sys.exit(main())
