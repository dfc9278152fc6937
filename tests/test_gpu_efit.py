"""DynamicsEnsemble.train_on_device: the ensemble trained on the GPU (amx_efit_step).

The comparator is the reference loop restated in torch on the CPU (tests/efit_ref.py) in fp64
(the yardstick) and fp32, on the index batches plan_batches draws (test_cpu_efit.py checks
those against real DataLoaders); G15 (tests/golden/make_golden_efit.py) is the reference's own
DynamicsEnsemble.train.  Tolerances: weights / biases / predictions
2e-5 * max(1, max|ref|); loss scalars 1e-4 relative; optimizer moments and buffers
1e-4 * max|ref| per tensor; step counts equal.  Every comparison first asserts that the fp32
comparator is within a quarter of the tolerance of fp64 (Adam's first steps are
lr * g / (|g| + eps): a near-zero gradient is a cliff, so the seeds must be ones where fp32
itself is stable), then that the device is within the tolerance of fp64."""
import copy

import numpy as np
import pytest
import torch

from efit_ref import events_from_plan, restate_member, synthetic_transitions

pytestmark = pytest.mark.gpu

TOL_W, TOL_LOSS, TOL_STATE = 2e-5, 1e-4, 1e-4
ADAM = {"optim": "adam", "lr": 1e-3, "eps": 1e-8}  # run.py's defaults


class Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def _np(t):
    return torch.as_tensor(t).detach().double().cpu().numpy()


def _err_w(x, ref):
    return float(np.abs(_np(x) - _np(ref)).max() / max(1.0, np.abs(_np(ref)).max()))


def _err_state(x, ref):
    return float(np.abs(_np(x) - _np(ref)).max() / max(np.abs(_np(ref)).max(), 1e-300))


def _err_loss(x, ref):
    return abs(float(x) - float(ref)) / abs(float(ref))


def _check(kind, name, dev, r32, r64):
    err, tol = {"w": (_err_w, TOL_W), "state": (_err_state, TOL_STATE), "loss": (_err_loss, TOL_LOSS)}[kind]
    e32, ed = err(r32, r64), err(dev, r64)
    print(f"{name}: fp32 {e32:.3e} device {ed:.3e} (tol {tol:.0e})")
    assert e32 <= 0.25 * tol, f"{name}: the fp32 comparator is {e32:.3e} from fp64 (precondition {0.25 * tol:.1e})"
    assert ed <= tol, f"{name}: device {ed:.3e} from fp64 (tol {tol:.1e})"


def _check_fixture(kind, name, dev, fixture, r64):
    """G15: the recorded reference run is the fp32 side of _check, and the device is also
    within the tolerance of the recording itself."""
    _check(kind, name, dev, fixture, r64)
    err, tol = {"w": (_err_w, TOL_W), "state": (_err_state, TOL_STATE), "loss": (_err_loss, TOL_LOSS)}[kind]
    assert err(dev, fixture) <= tol, f"{name}: device {err(dev, fixture):.3e} from the reference run (tol {tol:.1e})"


def _opt_key(optim):
    return ("exp_avg", "exp_avg_sq") if optim == "adam" else ("momentum_buffer",)


def make_ens(S, A, hidden, tr, va, optim_args, batch, transform=True, ctx=None, base_seed=100):
    from amp_extensions_amd.datasets import AmpDataset
    from amp_extensions_amd.ensemble import DynamicsEnsemble
    return DynamicsEnsemble(S, A, AmpDataset(*tr), AmpDataset(*va) if va is not None else None, num_models=4,
                            batch_size=batch, hidden_sizes=list(hidden), transform=transform, dense_connect=True,
                            optim_args=optim_args, base_seed=base_seed, device=torch.device("cpu"), ctx=ctx)


def restate(ens, tr, va, epochs, validate, grad_clip, seed, dtype):
    """Every member of `ens` (from its current host state) through the batches that
    train_on_device(seed) will draw; returns the per-member results of restate_member."""
    from amp_extensions_amd.ensemble import index_loader, materialise, plan_batches
    pg = ens.models[0].optimizer.param_groups[0]
    optim = "adam" if "eps" in pg else "sgd"
    lr, p1 = pg["lr"], pg["eps"] if optim == "adam" else pg["momentum"]
    n, nv, bs = tr[0].shape[0], (va[0].shape[0] if validate else 0), ens.batch_size
    torch.manual_seed(seed)
    plan, _ = plan_batches(n, nv, bs, epochs, ens.num_models, validate)
    tl, vl = index_loader(n, bs), (index_loader(nv, bs) if validate else None)
    data = {"train": tr, "val": va}
    if not validate:
        data.pop("val")
    out = []
    for g, m in enumerate(ens.models):
        ev = events_from_plan(plan[g], tl, vl, materialise)
        osd = copy.deepcopy(m.optimizer.state_dict())
        out.append(restate_member(copy.deepcopy(m.model.state_dict()), osd if osd["state"] else None,
                                  ens.transformations if ens.transform else None, data, ev, optim, lr, p1, grad_clip,
                                  dtype))
    return out


def epoch_averages(res, kind, steps_per_epoch):
    ls = [l for k, l in res["losses"] if k == kind]
    return [float(np.average(ls[i:i + steps_per_epoch])) for i in range(0, len(ls), steps_per_epoch)]


def compare_run(tag, ens, info, writer, r32, r64, epochs, validate, n, nv, optim, extra_steps=0):
    bs = ens.batch_size
    spe, spv = -(-n // bs), (-(-nv // bs) if validate else 0)
    for g, m in enumerate(ens.models):
        t32, t64 = epoch_averages(r32[g], "t", spe), epoch_averages(r64[g], "t", spe)
        _check("loss", f"{tag} m{g} train_min_loss", info[g][0], min(t32), min(t64))
        _check("loss", f"{tag} m{g} train_losses[0]", info[g][1], t32[0], t64[0])
        assert int(np.argmin(t32)) == int(np.argmin(t64))
        sd = m.model.state_dict()
        for k in sd:
            _check("w", f"{tag} m{g} {k}", sd[k], r32[g]["model"][k], r64[g]["model"][k])
        mine = m.optimizer.state_dict()["state"]
        for j, st64 in r64[g]["optim"]["state"].items():
            for key in _opt_key(optim):
                _check("state", f"{tag} m{g} p{j} {key}", mine[j][key], r32[g]["optim"]["state"][j][key], st64[key])
            if optim == "adam":
                assert float(mine[j]["step"]) == float(st64["step"]) == extra_steps + epochs * spe
    # the writer saw every epoch average of every member (epoch-major, train before validate)
    tr_rows = [r for r in writer.rows if r[0] == "Loss/train"]
    va_rows = [r for r in writer.rows if r[0] == "Loss/validate"]
    assert len(tr_rows) == epochs * len(ens.models) and len(va_rows) == (epochs * len(ens.models) if validate else 0)
    for e in range(epochs):
        for g in range(len(ens.models)):
            t32, t64 = epoch_averages(r32[g], "t", spe), epoch_averages(r64[g], "t", spe)
            row = tr_rows[e * len(ens.models) + g]
            assert row[2] == e
            _check("loss", f"{tag} m{g} epoch {e} train", row[1], t32[e], t64[e])
            if validate:
                v32, v64 = epoch_averages(r32[g], "v", spv), epoch_averages(r64[g], "v", spv)
                _check("loss", f"{tag} m{g} epoch {e} validate", va_rows[e * len(ens.models) + g][1], v32[e], v64[e])


# name: S, A, hidden, n, n_val, batch, optim_args, grad_clip, epochs, validate, transform, seed
CASES = {
    "a_adam_clip": (24, 6, [32, 32], 600, 300, 256, ADAM, 1.0, 2, True, True, 11),
    "b_sgd_wide": (197, 36, [256, 256, 256], 300, 0, 128, {"optim": "sgd", "lr": 0.05, "momentum": 0.9}, 0.0, 1,
                   False, True, 12),
    "c_ragged": (24, 6, [32, 32], 250, 0, 100, {"optim": "sgd", "lr": 0.1, "momentum": 0.9}, 0.25, 1, False, True, 13),
    "d_no_transform": (24, 6, [32, 32], 300, 0, 128, ADAM, 0.0, 1, False, False, 14),
}
CASE_POWER = {"a_adam_clip": 3}  # heavy-tailed inputs: the first-step gradient norm exceeds the clip


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(name):
    S, A, hidden, n, nv, batch, oa, clip, epochs, validate, transform, seed = CASES[name]
    power = CASE_POWER.get(name, 1)
    tr = synthetic_transitions(n, S, A, 100 + seed, power)
    va = synthetic_transitions(nv, S, A, 200 + seed, power) if nv else None
    ens = make_ens(S, A, hidden, tr, va, oa, batch, transform=transform)
    r64 = restate(ens, tr, va, epochs, validate, clip, seed, torch.float64)
    r32 = restate(ens, tr, va, epochs, validate, clip, seed, torch.float32)
    if name == "a_adam_clip":  # the clip is live
        assert all(r["first_norm"] > 1.0 for r in r64), [r["first_norm"] for r in r64]
    if name == "c_ragged":
        assert all(r["first_norm"] > clip for r in r64)
    torch.manual_seed(seed)
    w = Writer()
    info = ens.train_on_device(epochs, validate=validate, grad_clip=clip, writer=w)
    compare_run(name, ens, info, w, r32, r64, epochs, validate, n, nv, oa["optim"])
    assert ens.engine._fit is None  # the training state is released


def _g15_ens(g, block, ctx=None):
    S, A, hidden = int(g["S"]), int(g["A"]), [int(x) for x in g["hidden"]]
    tr = synthetic_transitions(int(g["n_train"]), S, A, int(g["seed_train"]))
    va = synthetic_transitions(int(g["n_val"]), S, A, int(g["seed_val"]))
    oa = ({"optim": "adam", "lr": float(g["adam_lr"]), "eps": float(g["adam_p1"])} if block == "adam" else
          {"optim": "sgd", "lr": float(g["sgd_lr"]), "momentum": float(g["sgd_p1"])})
    return make_ens(S, A, hidden, tr, va, oa, int(g["batch"]), ctx=ctx), tr, va


@pytest.mark.parametrize("block", ["adam", "sgd"])
def test_g15_reference_train(golden, block):
    """The reference's own DynamicsEnsemble.train(epochs=2, validate=True): returns, final
    weights, optimizer state, step count.  The sgd block's best epoch is not its last: the
    members still end with the last epoch's parameters (the reference's "best" dicts are views)."""
    g = golden("g15_ensemble_train.npz")
    ens, tr, va = _g15_ens(g, block)
    epochs, clip, seed = int(g["epochs"]), float(g[f"{block}_grad_clip"]), int(g[f"{block}_seed"])
    r64 = restate(ens, tr, va, epochs, True, clip, seed, torch.float64)
    ref_info = g[f"{block}_info"]
    if block == "sgd":
        assert (ref_info[:, 0] == ref_info[:, 1]).any()  # a member whose best epoch is not its last
    torch.manual_seed(seed)
    info = ens.train_on_device(epochs, validate=True, grad_clip=clip)
    spe = -(-int(g["n_train"]) // int(g["batch"]))
    for k, m in enumerate(ens.models):
        t64 = epoch_averages(r64[k], "t", spe)
        _check_fixture("loss", f"g15 {block} m{k} train_min_loss", info[k][0], ref_info[k][0], min(t64))
        _check_fixture("loss", f"g15 {block} m{k} train_losses[0]", info[k][1], ref_info[k][1], t64[0])
        params = list(m.model.parameters())
        names = list(m.model.state_dict())
        for j, p in enumerate(params):
            _check_fixture("w", f"g15 {block} m{k} {names[j]}", p, g[f"{block}_m{k}_p{j}"], r64[k]["model"][names[j]])
            st, st64 = m.optimizer.state[p], r64[k]["optim"]["state"][j]
            if block == "adam":
                _check_fixture("state", f"g15 adam m{k} p{j} exp_avg", st["exp_avg"], g[f"adam_m{k}_p{j}_exp_avg"],
                       st64["exp_avg"])
                _check_fixture("state", f"g15 adam m{k} p{j} exp_avg_sq", st["exp_avg_sq"], g[f"adam_m{k}_p{j}_exp_avg_sq"],
                       st64["exp_avg_sq"])
                assert float(st["step"]) == float(g[f"adam_m{k}_step"]) == epochs * spe
            else:
                _check_fixture("state", f"g15 sgd m{k} p{j} momentum_buffer", st["momentum_buffer"],
                       g[f"sgd_m{k}_p{j}_buf"], st64["momentum_buffer"])


S13, A13 = 226, 28


@pytest.fixture(scope="module")
def resumed(golden, golden_path, tmp_path_factory):
    """G13's checkpoint (Adam at step 1) loaded, a SimEnv built from the ensemble, then one
    epoch trained on the device."""
    import amp_extensions_amd as amx
    from test_gpu_ensemble_ckpt import synthetic_offline
    from test_gpu_simenv_dropin import RUN_PY_RESET_ARGS, write_deepmimic_tree
    g = golden("g13_ensemble_ckpt.npz")
    tr = tuple(torch.from_numpy(x).float() for x in synthetic_offline(int(g["n_offline"]), int(g["offline_seed"])))
    oa = {"optim": str(g["optim"]), "lr": float(g["lr"]), "eps": float(g["eps"])}
    hidden = [int(x) for x in g["hidden"]]
    ens = make_ens(S13, A13, hidden, tr, None, oa, 256)
    ens.load_ensemble(golden_path("g13_ensemble.pt"))
    args = write_deepmimic_tree(str(tmp_path_factory.mktemp("dm")))
    env = amx.SimEnv(deepmimic_args=args, dynamic_ensemble=ens, reset_args=RUN_PY_RESET_ARGS, seed=3)
    r64 = restate(ens, tr, None, 1, False, 1.0, 21, torch.float64)
    r32 = restate(ens, tr, None, 1, False, 1.0, 21, torch.float32)
    torch.manual_seed(21)
    w = Writer()
    info = ens.train_on_device(1, grad_clip=1.0, writer=w)
    return dict(ens=ens, tr=tr, r32=r32, r64=r64, info=info, writer=w, env=env, args=args, hidden=hidden, oa=oa,
                reset_args=RUN_PY_RESET_ARGS)


def test_resume_from_checkpoint(resumed):
    r = resumed
    compare_run("resume", r["ens"], r["info"], r["writer"], r["r32"], r["r64"], 1, False, r["tr"][0].shape[0], 0,
                "adam", extra_steps=1)


def test_inference_after_training(resumed, tmp_path):
    """The f16x3 inference path serves the trained weights: bit-equal to a fresh ensemble built
    from the synced host weights; save_ensemble -> load_ensemble round-trips model and
    optimizer state bit-identically; a SimEnv built before training steps with them."""
    import amp_extensions_amd as amx
    from amp_extensions_amd.ensemble import DynamicsEnsemble
    r = resumed
    ens = r["ens"]
    fresh = DynamicsEnsemble.from_weights(S13, A13, [m.model.layers() for m in ens.models], ens.transformations,
                                          hidden_sizes=r["hidden"], ctx=ens.ctx)
    qs, qa = r["tr"][0][:48], r["tr"][1][:48]
    for k in range(4):
        assert torch.equal(ens.models[k].forward(qs, qa), fresh.models[k].forward(qs, qa))
    p = str(tmp_path / "ensemble.pt")
    ens.save_ensemble(p)
    other = make_ens(S13, A13, r["hidden"], r["tr"], None, r["oa"], 256, ctx=ens.ctx, base_seed=7)
    other.load_ensemble(p)
    for m, o in zip(ens.models, other.models):
        for k, v in m.model.state_dict().items():
            assert torch.equal(o.model.state_dict()[k], v), k
        a, b = m.optimizer.state_dict(), o.optimizer.state_dict()
        assert a["param_groups"] == b["param_groups"] and set(a["state"]) == set(b["state"])
        for j, st in a["state"].items():
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
            for k, v in st.items():
                assert torch.equal(torch.as_tensor(b["state"][j][k]), torch.as_tensor(v)), (j, k)
    for k in range(4):
        assert torch.equal(other.models[k].forward(qs, qa), ens.models[k].forward(qs, qa))
    env2 = amx.SimEnv(deepmimic_args=r["args"], dynamic_ensemble=fresh, reset_args=r["reset_args"], seed=3)
    o1, o2 = r["env"].reset(), env2.reset()
    np.testing.assert_array_equal(o1, o2)
    act = np.random.RandomState(4).randn(A13) * 0.5
    n1, _, d1, _ = r["env"].step(act.copy())
    n2, _, d2, _ = env2.step(act.copy())
    np.testing.assert_array_equal(n1, n2)
    assert d1 == d2


def _pad_masks(eng):
    """Per layer (W mask [N_i][K_i], b mask [N_i]) of the valid (unpadded) entries."""
    masks = eng.layout.views(eng.layout.live_mask())
    return list(zip(masks[0::2], masks[1::2]))


def test_padding_stays_zero_and_fit_is_deterministic():
    """Engine level (the training state is inspectable between fit_begin and fit_end): padded
    weights, biases and optimizer state are exactly 0 after training; two trainings from the
    same state and batches are bit-identical."""
    S, A, hidden, n, batch = 24, 6, [32, 32], 250, 100
    tr = synthetic_transitions(n, S, A, 31)
    rs = np.random.RandomState(5)
    idx = np.stack([np.stack([rs.permutation(n)[:batch] for _ in range(3)]) for _ in range(4)]).astype(np.int32)
    sizes = [100, 100, 50]
    runs = []
    for optim, lr, p1 in (("adam", 1e-3, 1e-8), ("sgd", 0.05, 0.9)):
        for rep in range(2):
            ens = make_ens(S, A, hidden, tr, None, ADAM, batch)
            eng = ens.engine
            eng.fit_begin(tr, optim, lr, p1, batch)
            losses = [eng.fit_epoch(idx, sizes, train=True, grad_clip=1.0) for _ in range(2)]
            f = eng._fit
            state = dict(W=[w.cpu() for w in eng.W], b=[b.cpu() for b in eng.b], s1=f["s1"].cpu(),
                         s2=None if f["s2"] is None else f["s2"].cpu(), step=f["step"].cpu(), losses=losses)
            masks = _pad_masks(eng)
            for i, (Wm, bm) in enumerate(masks):
                assert not state["W"][i][:, ~Wm].any() and not state["b"][i][:, ~bm].any(), (optim, i)
                assert state["W"][i][:, Wm].abs().min() > 0
            for key in ("s1", "s2"):
                if state[key] is None:
                    continue
                views = eng.layout.views(state[key])
                for i, (Wv, bv) in enumerate(zip(views[0::2], views[1::2])):
                    assert not Wv[:, ~masks[i][0]].any() and not bv[:, ~masks[i][1]].any(), (optim, key, i)
                    assert Wv[:, masks[i][0]].abs().max() > 0
            assert state["step"].tolist() == [6] * 4
            eng.fit_end()
            runs.append(state)
        a, b = runs[-2], runs[-1]
        for x, y in zip(a["W"] + a["b"] + [a["s1"]] + a["losses"], b["W"] + b["b"] + [b["s1"]] + b["losses"]):
            assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


def test_refusals_allocate_nothing():
    from amp_extensions_amd.ensemble import DynamicsEnsemble
    S, A = 24, 6
    tr = synthetic_transitions(64, S, A, 41)
    ens = make_ens(S, A, [32, 32], tr, None, ADAM, 32)
    eng = ens.engine
    with pytest.raises(ValueError):  # a member count different from the context's M
        eng.fit_begin(tr, "adam", 1e-3, 1e-8, 32, num_models=3)
    with pytest.raises(NotImplementedError):  # unequal hidden widths
        eng.fit_begin(tr, "adam", 1e-3, 1e-8, 32, hidden_sizes=[32, 64])
    with pytest.raises(NotImplementedError):
        eng.fit_begin(tr, "rmsprop", 1e-3, 1e-8, 32)
    with pytest.raises(ValueError):
        eng.fit_begin(tr, "adam", 1e-3, 1e-8, 0)
    assert eng._fit is None
    with pytest.raises(ValueError):
        DynamicsEnsemble(S, A, ens.train_dataset, None, num_models=3, hidden_sizes=[32, 32], optim_args=ADAM,
                         ctx=ens.ctx)
    with pytest.raises(NotImplementedError):
        ens.train(1)


def test_t64_gemm_is_bit_identical_to_the_128_tile():
    """amx_gemm_bias_act_t64 (the training step's forward at few rows) runs every output
    element's K chain as amx_gemm_bias_act does: bit-equal, in place in the dense-concat
    buffer, several row / column tiles and groups, K not a multiple of the 64-wide tile."""
    from amp_extensions_amd import _native as N
    from amp_extensions_amd.engine import AmxContext
    ctx = AmxContext(24, 6, n_models=4, hidden=128, n_hidden=2)
    G, rows, K, Nn = 4, 256, 160, 128
    gen = torch.Generator().manual_seed(3)
    A0 = torch.randn(G, rows, K + Nn, generator=gen).cuda()
    W = torch.randn(G, Nn, K, generator=gen).cuda()
    b = torch.randn(G, Nn, generator=gen).cuda()
    outs = []
    for fn in (ctx.lib.amx_gemm_bias_act, ctx.lib.amx_gemm_bias_act_t64):
        A = A0.clone()
        N.check(fn(ctx.h, G, rows, Nn, K, A.data_ptr(), K + Nn, rows * (K + Nn), W.data_ptr(), K, Nn * K, b.data_ptr(),
                   Nn, A.data_ptr(), K + Nn, rows * (K + Nn), K, N.AMX_ACT_RELU, ctx.stream), "gemm")
        outs.append(A.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = torch.relu(torch.einsum("grk,gnk->grn", A0[:, :, :K].double().cpu(), W.double().cpu()) + b.double().cpu()[:, None])
    assert _err_w(outs[1][:, :, K:], ref) <= TOL_W
    assert torch.equal(outs[1][:, :, :K], A0[:, :, :K].cpu())


class Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def test_save_path_files_and_log_strings(tmp_path):
    """The reference's files under save_path (model{i}/final_model.pt, best_train_checkpoint.pt,
    best_validate_checkpoint.pt, the {epoch+1}_checkpoint.pt cadence: here epochs // 2 = 1) and
    its logger strings.  The "best" files hold the final parameters under the best epoch's
    number and loss, as the reference's view-valued best dicts do."""
    S, A, hidden, n, nv, batch, epochs = 24, 6, [32, 32], 600, 300, 256, 2
    tr, va = synthetic_transitions(n, S, A, 51), synthetic_transitions(nv, S, A, 52)
    ens = make_ens(S, A, hidden, tr, va, ADAM, batch)
    log = Logger()
    torch.manual_seed(5)
    info = ens.train_on_device(epochs, validate=True, logger=log, log_epoch=True, grad_clip=1.0,
                               save_path=str(tmp_path), save_checkpoints=True)
    spe = -(-n // batch)
    for g, m in enumerate(ens.models):
        d = tmp_path / f"model{g}"
        assert sorted(p.name for p in d.iterdir()) == ["1_checkpoint.pt", "best_train_checkpoint.pt",
                                                       "best_validate_checkpoint.pt", "final_model.pt"]
        files = {p.name: torch.load(str(p), map_location="cpu", weights_only=False) for p in d.iterdir()}
        for f in files.values():
            assert set(f) == {"model", "optim", "epoch", "loss"}
        mid, fin = files["1_checkpoint.pt"], files["final_model.pt"]
        assert mid["epoch"] == 1 and mid["loss"] == info[g][1]
        assert fin["epoch"] == epochs
        assert files["best_train_checkpoint.pt"]["loss"] == info[g][0]
        assert files["best_train_checkpoint.pt"]["epoch"] in (1, 2)
        sd = m.model.state_dict()
        for name in ("final_model.pt", "best_train_checkpoint.pt", "best_validate_checkpoint.pt"):
            for k, v in sd.items():
                assert torch.equal(files[name]["model"][k], v), (name, k)
            assert float(files[name]["optim"]["state"][0]["step"]) == epochs * spe
        assert float(mid["optim"]["state"][0]["step"]) == spe
        assert not torch.equal(mid["model"]["fc_layers.0.weight"], sd["fc_layers.0.weight"])
    M = len(ens.models)
    assert log.lines[:M] == [f">>>>Training Model {i + 1}/{M}" for i in range(M)]
    assert sum(l.startswith("Epoch: 0, Train Loss: ") for l in log.lines) == M
    assert sum(l.startswith("Epoch 1 Validation Loss: ") for l in log.lines) == M
    assert sum(l.startswith("Train: Dynamics Start | Best Loss | Epoch: ") for l in log.lines) == M
    assert sum(l.startswith("Validate: Dynamics Start | Best Loss | Epoch: ") for l in log.lines) == M
    assert f"Train: Dynamics Start | Best Loss | Epoch: {info[0][1]} | {info[0][0]} | " in log.lines[-2 * M]
