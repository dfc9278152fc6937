"""Plain (dense_connect=False) dynamics ensembles on the device: PlainDynamicsEnsemble, the
factory dynamics_ensemble and as_device_ensemble over the windowed f16x3 layers
(amx_gemm_bias_act_h3_win / amx_gemm_out_unnorm_h3_win) and the plain training step.

4 members, S/A = 197/36.  The comparators: an integer reference on exactly summable operands
(bit for bit), tests/plain_ref.py in fp64 with the reference's own fp32 torch forward as the
yardstick of the rounded forward, and G24 (tests/golden/make_golden_plain.py): the reference's
own save_ensemble files, run.py's load + compute_threshold sequence and train(epochs=2,
validate=True) of plain ensembles.  Training tolerances are test_gpu_efit.py's (G15's)."""
import copy

import numpy as np
import pytest
import torch

import plain_ref as PR
from efit_ref import events_from_plan, synthetic_transitions
from h3_exact import row_exponent
from oracle import milo_ref as R

pytestmark = pytest.mark.gpu

S, A, M = 197, 36, 4
DEV = "cuda"
ADAM = {"optim": "adam", "lr": 1e-3, "eps": 1e-8}


def offline_t(n, seed):
    from amp_extensions_amd.synthetic import offline
    return tuple(torch.from_numpy(x).float() for x in offline(n, S, A, seed))


def _rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max())


# ---- exact forward ----------------------------------------------------------------------------------
# Every operand is a small integer (or half-integer) times a power of two and every weight has one
# fp16 limb, so each layer's three-product sum is exact in fp32 in any order (at most 8 terms of
# < 2^17 granules: far below the 2^22 of tests/h3_exact.py) and the device must return the
# integer arithmetic's bits.  Window i's unit is 2^MAGS[i] (x0's is 1): a layer that scaled its
# rows by another window's exponent slot -- or by a max over the leading slots -- would flush
# them to zero or overflow fp16 (adjacent windows are 2^40 and more apart), and one that read
# another window would see other data.
MAGS = [-40, 40, -38]
NNZ = 8


def exact_case(hidden, B, seed):
    """Per member [(W, b), ...] in nn.Linear layout, the six normalizers, inputs (s, a) and the
    reference's x0, hidden outputs [L][M][B][h] and preds [M][B][S], all fp64 holding fp32 values."""
    rs = np.random.RandomState(seed)
    L, h = len(hidden), hidden[0]
    mags = MAGS[:L]
    mu_s, mu_a = rs.randint(-1, 2, S).astype(np.float64), rs.randint(-1, 2, A).astype(np.float64)
    sd_s, sd_a = np.exp2(rs.randint(-1, 2, S)), np.exp2(rs.randint(-1, 2, A))
    mu_d, sd_d = rs.randint(-3, 4, S).astype(np.float64), np.exp2(rs.randint(-1, 3, S))
    s, a = rs.randint(-3, 4, (B, S)).astype(np.float64), rs.randint(-3, 4, (B, A)).astype(np.float64)
    x0 = np.concatenate([(s - mu_s) / sd_s, (a - mu_a) / sd_a], 1)
    weights, hs, preds = [], [[] for _ in range(L)], []
    for _ in range(M):
        w, x, prev = [], x0, 0
        for i in range(L + 1):
            n, k = (S if i == L else h), x.shape[1]
            unit = np.exp2((0 if i == L else mags[i]) - prev)
            W = np.zeros((n, k))
            for r in range(n):
                W[r, rs.choice(k, NNZ, replace=False)] = rs.choice([-1.0, 1.0], NNZ)
            out_unit = np.exp2(0 if i == L else mags[i])
            b = rs.randint(-8, 25, n).astype(np.float64) * out_unit
            W *= unit
            y = x @ W.T + b
            w.append((W, b))
            if i < L:
                x = np.maximum(y, 0.0)
                hs[i].append(x)
                prev = mags[i]
            else:
                preds.append(y * sd_d + mu_d)
        weights.append(w)
    hs, preds = [np.stack(v) for v in hs], np.stack(preds)
    for v in [x0, preds] + hs:  # every value is a fp32 number: the integer arithmetic is the fp32 result
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    for i in range(L):  # the hidden windows are alive and a distinct magnitude each
        assert (hs[i] > 0).mean() > 0.3
    norms = (mu_s, sd_s, mu_a, sd_a, mu_d, sd_d)
    return weights, norms, (s, a), x0, hs, preds


@pytest.mark.parametrize("B", [128, 200])
@pytest.mark.parametrize("hidden", [[64, 64], [64] * 3], ids=["h64x2", "h64x3"])
def test_exact_forward_bits(hidden, B):
    """The device's x0, every hidden window, every row-exponent slot and preds equal the integer
    reference bit for bit; pad columns of the windows stay zero.  200 lanes pad to 256 rows."""
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    weights, norms, (s, a), x0, hs, preds = exact_case(hidden, B, 7 + len(hidden))
    tw = [[(torch.from_numpy(W).float(), torch.from_numpy(b).float()) for W, b in w] for w in weights]
    ens = PlainDynamicsEnsemble.from_weights(S, A, tw, [torch.from_numpy(x).float() for x in norms],
                                             hidden_sizes=hidden)
    eng = ens.engine
    assert eng.plain and eng.gemm == "f16x3"
    c = eng.ctx
    assert [tuple(w.shape[1:]) for w in eng.W] == [(c.Hp, c.k0_pad)] + [(c.Hp, c.Hp)] * (len(hidden) - 1) + \
        [(c.n_out_pad, c.Hp)]
    out = eng.forward_preds(torch.from_numpy(s).float().to(DEV), torch.from_numpy(a).float().to(DEV), B)
    torch.cuda.synchronize()
    ws = eng.workspace(B)
    assert ws["Bp"] == (128 if B == 128 else 256)
    act, rexp = ws["act"].cpu().numpy(), ws["rexp"].cpu().numpy()
    h = hidden[0]
    assert np.array_equal(act[0, :B, :S + A], x0.astype(np.float32))  # the shared x0: member 0's rows
    assert not act[0, :B, S + A:c.k0_pad].any()
    for i in range(len(hidden)):
        lo = c.k0_pad + i * c.Hp
        for m in range(M):
            assert np.array_equal(act[m, :B, lo:lo + h], hs[i][m].astype(np.float32)), (i, m)
            assert not act[m, :B, lo + h:lo + c.Hp].any(), (i, m)
            assert np.array_equal(rexp[m, i + 1, :B], row_exponent(hs[i][m])), (i, m)
    for m in range(M):
        assert np.array_equal(rexp[m, 0, :B], row_exponent(x0))
    # adjacent windows are far enough apart that the wrong slot cannot give the same bits
    e = np.stack([rexp[:, i, :B][rexp[:, i, :B] > -100].mean() for i in range(len(hidden) + 1)])
    assert (np.abs(np.diff(e)) >= 30).all(), e
    assert np.array_equal(out[:, :B].cpu().numpy(), preds.astype(np.float32))
    # the member-blocked forward (lane block g through member g alone): the same bits, row for row
    if B == 128:
        ob = torch.from_numpy(np.tile(s, (M, 1))).float().to(DEV)
        ac = torch.from_numpy(np.tile(a, (M, 1))).float().to(DEV)
        blk = eng.forward_blocked(ob, ac, B).cpu().numpy()
        for m in range(M):
            assert np.array_equal(blk[m * B:(m + 1) * B], preds[m].astype(np.float32)), m


# ---- rounded forward --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def offline512():
    from amp_extensions_amd.datasets import AmpDataset
    tr = offline_t(512, 24)
    return tr, AmpDataset(*tr).get_transformations(torch.device("cpu"))


@pytest.mark.parametrize("gemm", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("hidden", [[64, 64], [1024, 1024]], ids=["h64x2", "h1024x2"])
def test_rounded_forward_error_is_fp32s(offline512, hidden, gemm):
    """Seeded nn.Linear weights (the reference's init): the device's maximum absolute error over
    preds against the fp64 restatement is at most twice that of the reference's own fp32 torch
    forward of the same plain BasicMLP on the same rows (the two differ in the order of an
    fp32-accurate sum only).  That bound is the f16x3 default's.  The f32 and bf16x6 paths run one
    sequential fp32 chain over K (and bf16x6 drops three limb products of up to 2^-24 |a b| per
    term), whose error against a blocked CPU sum grows with K: they are held to the suite's
    forward tolerance for those paths, 2e-5, taken relative to max|preds| (these
    predictions are ~5e-3, so max(1, |ref|) would hide them).  Measured ratios: DESIGN §4."""
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble, init_ensemble_weights
    (s, a, _), norms = offline512
    B = 200
    s, a = s[:B], a[:B]
    w = init_ensemble_weights(S, A, hidden, M, 100, dense_connect=False)
    ens = PlainDynamicsEnsemble.random_init(S, A, norms, hidden_sizes=hidden, num_models=M, base_seed=100, gemm=gemm)
    for m, wm in zip(ens.models, w):
        for lin, (W, b) in zip(m.model.fc_layers, wm):
            assert torch.equal(lin.weight.data, W) and torch.equal(lin.bias.data, b)
    r64 = torch.stack([PR.forward(wm, norms, s, a, torch.float64) for wm in w]).numpy()
    r32 = torch.stack([PR.forward(wm, norms, s, a, torch.float32) for wm in w]).numpy()
    dev = ens.engine.forward_preds(s.to(DEV), a.to(DEV), B)[:, :B].cpu().numpy()
    e32, ed = float(np.abs(r32 - r64).max()), float(np.abs(dev - r64).max())
    print(f"plain {hidden} {gemm}: fp32 torch {e32:.3e} device {ed:.3e} ratio {ed / e32:.3f} "
          f"(max|preds| {np.abs(r64).max():.3f})")
    if gemm == "f16x3":
        assert ed <= 2.0 * e32, (ed, e32)
    else:
        assert ed <= 2e-5 * float(np.abs(r64).max()), (ed, float(np.abs(r64).max()))
    for k in range(M):  # models[k].forward serves the same rows
        assert torch.equal(ens.models[k].forward(s, a), torch.from_numpy(dev[k]))


# ---- G24: the reference's own checkpoints --------------------------------------------------------
@pytest.fixture(scope="module")
def run_py(golden, golden_path, offline512):
    """run.py:42-43, 54-57, 68-78, 108 with the factory bound as INTEGRATION §1 says and no
    --dynamic_dense_connect: construct, load_ensemble, compute_threshold."""
    from amp_extensions_amd.datasets import AmpDataset
    from amp_extensions_amd.ensemble import dynamics_ensemble as DynamicsEnsemble
    g = golden("g24_plain.npz")
    assert int(g["n_offline"]) == 512 and int(g["offline_seed"]) == 24
    (s, a, s2), _ = offline512
    device = torch.device("cpu")
    offline_dataset = AmpDataset(s, a, s2, device)
    optim_args = {"optim": "adam", "lr": float(g["adam_lr0"]), "eps": float(g["adam_eps0"])}
    dynamic_ensemble = DynamicsEnsemble(S, A, offline_dataset, None,
                                        num_models=4,
                                        batch_size=256, hidden_sizes=[int(x) for x in g["ck_hidden"]],
                                        transform=True,
                                        dense_connect=False, optim_args=optim_args,
                                        base_seed=int(g["base_seed"]), device=device)
    dynamic_ensemble.load_ensemble(golden_path("g24_plain_adam.pt"))
    dynamic_ensemble.compute_threshold()
    return g, dynamic_ensemble


def test_run_py_sequence_matches_reference(run_py):
    """Member forwards 2e-5 of max(1, |ref|), disagreement and threshold rel 1e-4: the tolerances
    test_gpu_ensemble_ckpt.py applies to the dense ensemble."""
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    g, ens = run_py
    assert type(ens) is PlainDynamicsEnsemble and ens.engine.plain
    print(f"threshold {ens.threshold!r} reference {float(g['threshold'])!r}")
    assert abs(ens.threshold - float(g["threshold"])) <= 1e-4 * abs(float(g["threshold"]))
    qs, qa = torch.from_numpy(g["query_s"]), torch.from_numpy(g["query_a"])
    for k, m in enumerate(ens.models):
        out = m.forward(qs, qa)
        assert out.device == torch.device("cpu")
        assert _rel(out.numpy(), g["preds"][k]) <= 2e-5
        assert _rel(m.forward(qs, qa, unnormalize_out=False).numpy(), g["preds_norm"][k]) <= 2e-5
    d = ens.get_action_discrepancy(qs, qa)
    np.testing.assert_allclose(d.numpy(), g["disc"], rtol=1e-4, atol=1e-4 * float(np.abs(g["disc"]).max()))
    assert torch.equal(d, ens.compute_discrepancy(qs, qa))


def _assert_same_checkpoint(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"model", "optim"}
        assert list(x["model"]) == list(y["model"])
        for k, v in x["model"].items():
            assert torch.equal(y["model"][k], v), k
        assert x["optim"]["param_groups"] == y["optim"]["param_groups"]
        assert set(x["optim"]["state"]) == set(y["optim"]["state"]) and len(x["optim"]["state"]) == 6
        for j, st in x["optim"]["state"].items():
            assert set(st) == set(y["optim"]["state"][j])
            for k, v in st.items():
                assert torch.equal(torch.as_tensor(y["optim"]["state"][j][k]), torch.as_tensor(v)), (j, k)


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_checkpoint_round_trip(run_py, golden_path, tmp_path, optim):
    """The reference's save_ensemble file loads (model and optimizer state, Adam's and
    SGD-Nesterov's) and save_ensemble writes a file whose tensors equal it bit for bit."""
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    g, ens0 = run_py
    oa = ADAM if optim == "adam" else {"optim": "sgd", "lr": float(g["sgd_lr0"]), "momentum": float(g["sgd_momentum0"])}
    ens = PlainDynamicsEnsemble(S, A, ens0.train_dataset, None, num_models=4,
                                hidden_sizes=[int(x) for x in g["ck_hidden"]], optim_args=oa, base_seed=7, ctx=ens0.ctx)
    src = golden_path(f"g24_plain_{optim}.pt")
    ens.load_ensemble(src)
    ref = torch.load(src, map_location="cpu", weights_only=True)
    key = "exp_avg" if optim == "adam" else "momentum_buffer"
    assert all(key in st for sd in ref for st in sd["optim"]["state"].values())
    _assert_same_checkpoint(ref, [m.get_state_dicts() for m in ens.models])
    p = str(tmp_path / "ensemble.pt")
    ens.save_ensemble(p)
    _assert_same_checkpoint(ref, torch.load(p, map_location="cpu", weights_only=True))
    if optim == "adam":  # the same file through either object: the same device results
        qs, qa = torch.from_numpy(g["query_s"]), torch.from_numpy(g["query_a"])
        for k in range(4):
            assert torch.equal(ens.models[k].forward(qs, qa), ens0.models[k].forward(qs, qa))


def test_reference_object_drops_in(run_py, offline512):
    """as_device_ensemble on the reference's object with plain members (it reads
    BasicMLP.dense_connect): the drop-in's bits; get_bonus_costs through either is torch.equal."""
    import amp_extensions_amd as amx
    from amp_extensions_amd.ensemble import BasicMLPWeights, as_device_ensemble
    from test_gpu_ensemble_ckpt import _ReferenceLikeEnsemble
    g, ens = run_py
    _, norms = offline512
    hidden = [int(x) for x in g["ck_hidden"]]
    models = []
    for m in ens.models:
        b = BasicMLPWeights(S + A, S, hidden, dense_connect=False)
        b.load_state_dict(m.model.state_dict())
        models.append(b)
    ref_obj = _ReferenceLikeEnsemble(S, A, models, norms, ens.threshold)
    dev = as_device_ensemble(ref_obj)
    assert dev.plain and as_device_ensemble(ref_obj) is dev
    qs, qa = torch.from_numpy(g["query_s"]).to(DEV), torch.from_numpy(g["query_a"]).to(DEV)
    assert torch.equal(dev.get_action_discrepancy(qs, qa), ens.engine.get_action_discrepancy(qs, qa))
    assert dev.threshold == ens.threshold
    s, _, s2 = offline_t(512, 3)
    cost = amx.RBFLinearCost(torch.cat([s, s2], 1), feature_dim=512, lambda_b=0.0025, seed=100, ctx=ens.ctx)
    ps, pa, ps2 = offline_t(96, 4)
    cost.fit_cost(torch.cat([ps, ps2], 1))
    c1, _ = cost.get_bonus_costs(ps, pa, ref_obj, next_states=ps2)
    c2, _ = cost.get_bonus_costs(ps, pa, ens, next_states=ps2)
    assert torch.equal(c1, c2)


# ---- G24: the reference's own training run -------------------------------------------------------
def _restate(ens, tr, va, epochs, clip, seed, dtype):
    from amp_extensions_amd.ensemble import index_loader, materialise, plan_batches
    pg = ens.models[0].optimizer.param_groups[0]
    optim = "adam" if "eps" in pg else "sgd"
    lr, p1 = pg["lr"], pg["eps"] if optim == "adam" else pg["momentum"]
    n, nv, bs = tr[0].shape[0], va[0].shape[0], ens.batch_size
    torch.manual_seed(seed)
    plan, _ = plan_batches(n, nv, bs, epochs, ens.num_models, True)
    tl, vl = index_loader(n, bs), index_loader(nv, bs)
    return [PR.restate_member(copy.deepcopy(m.model.state_dict()), None, ens.transformations, {"train": tr, "val": va},
                              events_from_plan(plan[g], tl, vl, materialise), optim, lr, p1, clip, dtype)
            for g, m in enumerate(ens.models)]


@pytest.mark.parametrize("block", ["adam", "sgd"])
def test_g24_reference_train(golden, block):
    """The reference's DynamicsEnsemble.train(epochs=2, validate=True) of a plain [64, 64]
    ensemble, batch 64 (batches of 64, 64, 64, 8): the returned losses, final weights, optimizer
    state and step count within G15's tolerances; then the inference images, refreshed in place:
    the engine built before training predicts with the trained weights."""
    from amp_extensions_amd.datasets import AmpDataset
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    from test_gpu_efit import _check_fixture, epoch_averages
    g = golden("g24_plain.npz")
    files = {k: golden(f"g24_train_{block}_{k}.npz") for k in (("w", "s1", "s2") if block == "adam" else ("w", "s1"))}
    hidden, batch = [int(x) for x in g["tr_hidden"]], int(g["batch"])
    assert hidden == [64, 64] and batch == 64 and int(g["epochs"]) == 2
    tr = synthetic_transitions(int(g["n_train"]), S, A, int(g["seed_train"]))
    va = synthetic_transitions(int(g["n_val"]), S, A, int(g["seed_val"]))
    oa = ({"optim": "adam", "lr": float(g["adam_lr"]), "eps": float(g["adam_p1"])} if block == "adam" else
          {"optim": "sgd", "lr": float(g["sgd_lr"]), "momentum": float(g["sgd_p1"])})
    ens = PlainDynamicsEnsemble(S, A, AmpDataset(*tr), AmpDataset(*va), num_models=4, batch_size=batch,
                                hidden_sizes=hidden, transform=True, optim_args=oa, base_seed=int(g["base_seed"]),
                                device=torch.device("cpu"))
    eng = ens.engine
    ptrs = [t.data_ptr() for t in eng.W2 + eng.wexp + eng.W + eng.b]
    qs, qa = tr[0][:48], tr[1][:48]
    before = [ens.models[k].forward(qs, qa) for k in range(4)]
    epochs, clip, seed = int(g["epochs"]), float(g[f"{block}_grad_clip"]), int(g[f"{block}_seed"])
    r64 = _restate(ens, tr, va, epochs, clip, seed, torch.float64)
    ref_info = g[f"{block}_info"]
    torch.manual_seed(seed)
    info = ens.train_on_device(epochs, validate=True, grad_clip=clip)
    spe = -(-int(g["n_train"]) // batch)
    assert spe == 4
    for k, m in enumerate(ens.models):
        t64 = epoch_averages(r64[k], "t", spe)
        _check_fixture("loss", f"g24 {block} m{k} train_min_loss", info[k][0], ref_info[k][0], min(t64))
        _check_fixture("loss", f"g24 {block} m{k} train_losses[0]", info[k][1], ref_info[k][1], t64[0])
        names = list(m.model.state_dict())
        for j, p in enumerate(m.model.parameters()):
            tag = f"m{k}_p{j}"
            _check_fixture("w", f"g24 {block} {tag} {names[j]}", p, files["w"][tag], r64[k]["model"][names[j]])
            st, st64 = m.optimizer.state[p], r64[k]["optim"]["state"][j]
            if block == "adam":
                _check_fixture("state", f"g24 adam {tag} exp_avg", st["exp_avg"], files["s1"][tag], st64["exp_avg"])
                _check_fixture("state", f"g24 adam {tag} exp_avg_sq", st["exp_avg_sq"], files["s2"][tag],
                               st64["exp_avg_sq"])
                assert float(st["step"]) == float(g[f"adam_m{k}_step"]) == epochs * spe
            else:
                _check_fixture("state", f"g24 sgd {tag} momentum_buffer", st["momentum_buffer"], files["s1"][tag],
                               st64["momentum_buffer"])
    assert eng._fit is None
    assert [t.data_ptr() for t in eng.W2 + eng.wexp + eng.W + eng.b] == ptrs  # refreshed in place
    fresh = PlainDynamicsEnsemble.from_weights(S, A, [m.model.layers() for m in ens.models], ens.transformations,
                                               hidden_sizes=hidden, ctx=ens.ctx)
    for k in range(4):
        after = ens.models[k].forward(qs, qa)
        assert torch.equal(after, fresh.models[k].forward(qs, qa))
        assert not torch.equal(after, before[k])
        want = PR.forward(ens.models[k].model.state_dict(), ens.transformations, qs, qa, torch.float64)
        assert _rel(after.numpy(), want.numpy()) <= 2e-5


def test_padding_stays_zero_after_training():
    """Zero-padded weights, biases and optimizer state of the windowed layout see a zero
    gradient: exactly 0 after Adam steps with the clip live."""
    from amp_extensions_amd.datasets import AmpDataset
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    tr = synthetic_transitions(200, S, A, 31)
    ens = PlainDynamicsEnsemble(S, A, AmpDataset(*tr), None, num_models=4, batch_size=64, hidden_sizes=[64] * 3,
                                optim_args=ADAM)
    eng = ens.engine
    rs = np.random.RandomState(5)
    idx = np.stack([np.stack([rs.permutation(200)[:64] for _ in range(2)]) for _ in range(4)]).astype(np.int32)
    eng.fit_begin(tr, "adam", 1e-3, 1e-8, 64)
    losses = eng.fit_epoch(idx, [64, 40], train=True, grad_clip=0.5)
    assert np.isfinite(losses).all() and losses.shape == (4, 2)
    f = eng._fit
    live = eng.layout.live_mask()
    W = torch.cat([t.cpu().reshape(4, -1) for Wb in zip(eng.W, eng.b) for t in Wb], 1)
    for name, v in (("W", W), ("s1", f["s1"].cpu()), ("s2", f["s2"].cpu())):
        assert not v[:, ~live].any(), name
        assert (v[:, live] != 0).float().mean() > 0.5, name
    assert f["step"].cpu().tolist() == [2] * 4
    eng.fit_end()


# ---- the same engine, both connectivities ---------------------------------------------------------
@pytest.fixture(scope="module")
def plain64(offline512):
    import amp_extensions_amd as amx
    from amp_extensions_amd.ensemble import PlainDynamicsEnsemble
    _, norms = offline512
    ens = PlainDynamicsEnsemble.random_init(S, A, norms, hidden_sizes=(64, 64), num_models=M, base_seed=100)
    pw, log_std = R.init_policy_weights(S, A, (32, 32), seed=100, init_log_std=-0.25)
    return amx, ens, pw, log_std


def test_sample_points_member_blocked_and_all_member(plain64):
    """sample_points(mode='trajectories'), 4 trajectories, horizon 8: member-blocked lanes
    (forward_blocked over the windows) against every member on every lane -- the same paths and
    shapes, states within test_gpu_sampler.py's tolerance for that pair -- and the first step of
    every path against the fp64 restatement of the trajectory's member."""
    from amp_extensions_amd.synthetic import reset_table
    from test_gpu_sampler import _state_close
    amx, ens, pw, log_std = plain64
    pol = amx.DevicePolicy(ens.ctx, pw, log_std)
    table = reset_table(256, S, 3)
    env = amx.BatchedSimEnv(ens, table, lanes=512, horizon=8, record_means=True)
    a = amx.sample_points(env, pol, num_to_collect=4, base_seed=5, num_workers=2, mode="trajectories",
                          member_blocked=False)
    b = amx.sample_points(env, pol, num_to_collect=4, base_seed=5, num_workers=2, mode="trajectories",
                          member_blocked=True)
    assert len(a) == len(b) == 4
    for i, (p, q) in enumerate(zip(b, a)):
        assert set(p) == set(q)
        for k in ("observations", "next_observations", "actions", "rewards"):
            assert p[k].shape == q[k].shape and p[k].dtype == q[k].dtype, (i, k)
        assert 1 <= len(p["rewards"]) <= 8 and p["observations"].shape[1] == S and p["actions"].shape[1] == A
        np.testing.assert_array_equal(p["observations"][0], q["observations"][0])
        _state_close(p["observations"], q["observations"], f"path {i} observations")
        _state_close(p["next_observations"], q["next_observations"], f"path {i} next_observations")
        np.testing.assert_allclose(p["actions"], q["actions"], rtol=0, atol=2e-4)
    # worker w's trajectory j = 1, 2 runs member j % M (SimEnv's reset counter, sim_env.py:282-283)
    for i, p in enumerate(b):
        k = (1 + i % 2) % M
        s0, a0 = torch.from_numpy(p["observations"][:1]).float(), torch.from_numpy(p["actions"][:1]).float()
        want = p["observations"][0] + PR.forward(ens.models[k].model.state_dict(), ens.transformations, s0, a0,
                                                 torch.float64).numpy()[0]
        _state_close(p["next_observations"][0], want, f"path {i} first step")


def test_graph_replay_matches_eager_rollouts(plain64):
    """RolloutEngine.graph_rollout at 256 lanes x 2 steps over a plain ensemble: the replay's
    lane states, actions, rewards and mb_mmd equal the eager rollouts' bit for bit."""
    from amp_extensions_amd.synthetic import expert, reset_table
    amx, ens, pw, log_std = plain64
    B, K = 256, 2
    ex = torch.from_numpy(expert(300, S, 3))
    table = reset_table(64, S, 1)
    runs = []
    for graph in (False, True):
        cost = amx.RBFLinearCost(ex, feature_dim=512, bw_quantile=0.1, bw_samples=5000, lambda_b=0.0025, seed=100,
                                 ctx=ens.ctx)
        pol = amx.DevicePolicy(ens.ctx, pw, log_std, seed=1)
        eng = amx.RolloutEngine(ens.engine, table, lanes=B, policy=pol, cost=cost, seed=2, max_steps=K)
        eng.reset_all()
        eng.rollout()
        eng.relabel()
        out = []
        if graph:
            replay = eng.graph_rollout(K, tail=cost.get_expert_cost)
            for _ in range(2):
                replay()
                out.append([x.clone() for x in (eng.obs, eng.acts, eng.rewards, eng.mb_mmd)])
        else:
            for _ in range(2):
                eng.rollout()
                eng.relabel()
                cost.get_expert_cost()
                out.append([x.clone() for x in (eng.obs, eng.acts, eng.rewards, eng.mb_mmd)])
        torch.cuda.synchronize()
        runs.append(out)
    for ea, eb in zip(*runs):
        for xa, xb in zip(ea, eb):
            assert torch.equal(xa, xb)
    assert torch.isfinite(runs[1][-1][0]).all() and not torch.equal(runs[1][0][1], runs[1][1][1])


def test_gemm_timer_spans_the_plain_forward(plain64):
    """amx_set_gemm_timer over a plain chain: one start stamp (layer 0) and one tick sum per
    forward -- every plain layer reads one exponent slot, so the windowed entry points carry the
    first-layer flag explicitly -- and the results are unchanged."""
    amx, ens, pw, log_std = plain64
    e, ctx = ens.engine, ens.ctx
    s, a, _ = offline_t(640, 9)
    ob, ac = s.to(DEV), a.to(DEV)
    ref = e.forward_preds(ob, ac, 640).clone()
    timer = ctx.gemm_timer()
    try:
        for _ in range(3):
            out = e.forward_preds(ob, ac, 640)
        torch.cuda.synchronize()
        t = timer.cpu().tolist()
    finally:
        ctx.gemm_timer(False)
    assert torch.equal(out, ref)
    assert t[1] == 0 and t[3] == 3 and t[2] > 0, t
    # a forward's ticks (100 MHz) span its L + 1 launches: more than one launch's few microseconds
    print(f"plain [64, 64] forward at 640 lanes: {t[2] / t[3] / 100:.1f} us in-kernel")


# ---- refusals ---------------------------------------------------------------------------------------
def test_refusals(run_py):
    from amp_extensions_amd.ensemble import DynamicsEnsemble, PlainDynamicsEnsemble
    _, ens = run_py
    for kw in (dict(use_resnet=True), dict(activation="tanh")):
        with pytest.raises(NotImplementedError):
            PlainDynamicsEnsemble(S, A, ens.train_dataset, None, hidden_sizes=[32, 32], ctx=ens.ctx, **kw)
    with pytest.raises(NotImplementedError):
        PlainDynamicsEnsemble(S, A, ens.train_dataset, None, hidden_sizes=[32, 64], ctx=ens.ctx)
    with pytest.raises(ValueError):
        PlainDynamicsEnsemble(S, A, ens.train_dataset, None, hidden_sizes=[32, 32], dense_connect=True, ctx=ens.ctx)
    with pytest.raises(NotImplementedError):
        DynamicsEnsemble(S, A, ens.train_dataset, None, hidden_sizes=[32, 32], dense_connect=False)
    with pytest.raises(ValueError):  # a plain context does not serve dense-connect members
        DynamicsEnsemble(S, A, ens.train_dataset, None, hidden_sizes=[32, 32], dense_connect=True, ctx=ens.ctx)
    with pytest.raises(NotImplementedError):
        ens.train(1)
