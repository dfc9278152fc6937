"""MLPCost on the device (amx_mlp_features_h3, MlpMap, costs.MLPCost) against the fp64
restatement of the reference's MLPCost on the same weights, at bounds measured in units of the
reference's own fp32 error on each test's rows (tests/mlpcost_ref.py states them and why the
usual 1e-4 relative gate does not fit this cost)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpcost_ref as M  # noqa: E402

from oracle import milo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def f64(t):
    return t.detach().double().cpu().numpy()


def make_ensemble(amx, S, A, feat_dim, hidden=(64, 64, 64, 64), n_offline=2048, seed=0):
    """The G5 stand-in at any (S, A): the oracle's seeded 4-member dense ensemble on synthetic
    offline rows, its threshold computed on the device."""
    s, a, s2 = M.synthetic_rows(n_offline, seed, S, A)
    norms = R.get_transformations(s, a, s2)
    ens_w = R.init_ensemble_weights(S, A, list(hidden), 4, 100)
    ctx = amx.AmxContext(S, A, n_models=4, hidden=hidden[0], n_hidden=len(hidden), feat_dim=feat_dim, device=DEV)
    ens = amx.DeviceEnsemble(ctx, ens_w, norms)
    ens.compute_threshold(s.to(DEV), a.to(DEV))
    return ctx, ens


def check_cost_against_fp64(cost, ref, y, x_pi, report):
    """phi, phi_e, w, mb_mmd, costs and the expert cost of a fitted device cost within the bounds."""
    phi_pi = f64(cost.get_rep(x_pi))
    e_phi = max(np.abs(phi_pi - ref.rep(x_pi)).max(), np.abs(f64(cost.expert_rep) - ref.expert_rep).max())
    mmd_dev = cost.fit_cost(x_pi)
    mmd = ref.fit_cost(x_pi)
    e_phi_e = np.abs(f64(cost.phi_e) - ref.phi_e).max()
    e_w = np.abs(f64(cost.w) - ref.w).max()
    print(f"[{report}] phi err {e_phi:.2e} (fp32 yardstick {y.phi_err:.2e})  phi_e err {e_phi_e:.2e} "
          f"({y.phi_e_err:.2e})  w err {e_w:.2e} ({y.w_err:.2e})  mb_mmd rel {abs(mmd_dev - mmd) / mmd:.1e}")
    assert e_phi <= y.d_phi
    assert e_phi_e <= y.d_phi_e
    assert e_w <= y.d_w
    assert abs(mmd_dev - mmd) <= M.mmd_bound(ref.w, y.d_w)
    row = M.dot_bound(ref.rep(x_pi), ref.w, y.d_phi, y.d_w)
    costs = f64(cost.get_costs(x_pi))
    assert costs.shape == (x_pi.shape[0], 1)
    assert (np.abs(costs[:, 0] - ref.get_costs(x_pi)) <= row).all()
    if ref.cost_range is not None:
        erow = M.dot_bound(ref.expert_rep, ref.w, y.d_phi, y.d_w)
        want = ref.expert_cost()
        assert abs(float(cost.get_expert_cost()) - want) <= (1 - ref.lam) * erow.mean() + M.ulp4(want)
    return row


# ---- G22: the reference's own records, all variants ------------------------------------------
@pytest.mark.parametrize("name", sorted(M.G22))
def test_g22_against_reference_and_fp64(golden, name):
    """Weights and bandwidth bit-equal to the reference's; phi, phi_e, w, mb_mmd, costs, the bonus
    cost with its info dict and the expert cost within the bounds of the fp64 restatement; the
    ensemble stand-in's threshold and weighted bonus against the reference ensemble's (G5's
    tolerance)."""
    import amp_extensions_amd as amx
    from amp_extensions_amd.costs import device_discrepancy
    g = golden("g22_mlp_cost.npz")
    cfg, C = M.G22[name], M.G22_COMMON
    S, A = cfg["S"], cfg["A"]
    ctx, ens = make_ensemble(amx, S, A, cfg["feature_dim"], C["ens_hidden"], C["n_offline"], C["offline_seed"])
    es, ea, es2 = M.synthetic_rows(C["n_expert"], C["expert_seed"], S, A)
    ps, pa, ps2 = M.synthetic_rows(C["n_pi"], C["pi_seed"], S, A, shift=C["pi_shift"])
    expert, x_pi = M.cost_rows(cfg["input_type"], es, ea, es2), M.cost_rows(cfg["input_type"], ps, pa, ps2)
    cost = amx.MLPCost(expert, hidden_dims=list(cfg["hidden_dims"]), activation="relu", feature_dim=cfg["feature_dim"],
                       input_type=cfg["input_type"], cost_range=cfg["cost_range"], bw_quantile=C["bw_quantile"],
                       bw_samples=C["bw_samples"], lambda_b=C["lambda_b"], seed=C["seed"], ctx=ctx)
    pre = f"{name}__sd__"
    want_sd = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
    sd = cost.net.state_dict()
    assert set(sd) == set(want_sd)
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), want_sd[k]), k
    assert cost.bw == float(g[f"{name}__bw"])
    assert cost.map.W2 is not None and cost.map.Kp % 32 == 0 and cost.map.D == x_pi.shape[1]

    ref = M.Ref64(want_sd, expert, cfg["feature_dim"], cfg["cost_range"], C["lambda_b"])
    ref.fit_cost(x_pi)
    y = M.Yardstick(ref, expert, x_pi)
    row = check_cost_against_fp64(cost, ref, y, x_pi, f"g22 {name}")

    bc, info = cost.get_bonus_costs(ps.to(DEV), pa.to(DEV), ens, next_states=ps2.to(DEV))
    disc = f64(device_discrepancy(ens, ps.to(DEV), pa.to(DEV)))
    c64, ipm64, wb64 = ref.bonus_costs(x_pi, disc, ens.threshold)
    lam = ref.lam
    slack = M.ulp4(ipm64, wb64)
    assert (np.abs(f64(info["ipm"])[:, 0] - ipm64) <= (1 - lam) * row + slack).all()
    assert (np.abs(f64(info["bonus"])[:, 0] - wb64) <= slack).all()
    assert (np.abs(f64(bc)[:, 0] - c64) <= (1 - lam) * row + slack).all()
    assert (np.abs(f64(info["v_targ"])[:, 0] - ref.get_costs(x_pi)) <= row).all()
    assert torch.equal(info["cost"], bc)
    # the stand-in ensemble is the reference's: threshold and weighted bonus as G5 checks them
    np.testing.assert_allclose(ens.threshold, float(g[f"{name}__threshold"]), rtol=1e-4)
    np.testing.assert_allclose(f64(info["bonus"]), g[f"{name}__bonus"], rtol=1e-4, atol=1e-7)
    if cfg["cost_range"] is None:
        with pytest.raises(TypeError):
            cost.get_expert_cost()


# ---- the feature layer alone, through the C ABI, one shape per tile family --------------------
def _tile_cases():
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    # F 512: (rows / 128) * 4 tiles of 128 x 128
    return [("below_n_cus_128x64", 256, 64, False),
            ("one_to_two_rounds_128x128", 32 * n_cus, 64, False),
            ("above_two_rounds_three_per_cu", 128 * (n_cus // 2 + 2), 64, True),
            ("whole_rounds_160x256", 80 * n_cus, 64, False),
            ("k_not_multiple_of_32", 256, 48, False)]


@pytest.mark.parametrize("case", _tile_cases(), ids=lambda c: c[0])
def test_feature_layer_every_tile_family(case):
    """amx_mlp_features_h3 on random [rows, K] inputs at one shape per tile family its dispatch
    rule (amx_rff_features_h3's) reaches on this device: phi against cos(tanh(x W^T + b)) scale in
    fp64 at the phi bound (4 x the torch-CPU fp32 error on the same rows), the column partials
    against the fp64 sums of the device's own phi rows over the valid rows of each 32-row group
    (n_valid in every case, a row mask in one)."""
    import amp_extensions_amd as amx
    _, rows, K, masked = case
    F = 512
    ctx = amx.AmxContext(24, 6, n_models=1, hidden=128, n_hidden=1, feat_dim=F, device=DEV)
    lib, h, st = ctx.lib, ctx.h, ctx.stream
    gen = torch.Generator().manual_seed(rows + K)
    x = (0.5 * torch.randn(rows, K, generator=gen)).float()
    W = (0.25 * torch.randn(F, K, generator=gen)).float()     # z = x W^T + b ~ N(0, 1): tanh's whole range
    b = (0.5 * torch.randn(F, generator=gen)).float()
    mask = (torch.rand(rows, generator=gen) > 0.1).to(torch.uint8) if masked else None
    n_valid = rows - 77
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    md = mask.to(DEV) if masked else None
    W2 = torch.empty(F * 2 * K, dtype=torch.int16, device=DEV)
    wexp = torch.empty(F, dtype=torch.int32, device=DEV)
    rexp = torch.empty(rows, dtype=torch.int32, device=DEV)
    assert lib.amx_split_f16x2(h, 1, F, K, Wd.data_ptr(), K, 0, W2.data_ptr(), F * 2 * K, wexp.data_ptr(), F, st) == 0
    assert lib.amx_row_exponents(h, 1, rows, K, xd.data_ptr(), K, 0, rexp.data_ptr(), rows, 1, st) == 0
    scale = float(np.float32(np.sqrt(2.0 / F)))
    phi = torch.empty(rows, F, device=DEV)
    part = torch.empty(rows // 32, F, dtype=torch.float64, device=DEV)
    assert lib.amx_mlp_features_h3(h, rows, n_valid, F, K, xd.data_ptr(), K, W2.data_ptr(), wexp.data_ptr(),
                                   rexp.data_ptr(), bd.data_ptr(), ctypes.c_float(scale), phi.data_ptr(), F,
                                   part.data_ptr(), None if md is None else md.data_ptr(), st) == 0
    torch.cuda.synchronize()
    phi, part = phi.double().cpu().numpy(), part.cpu().numpy()
    z64 = x.double().numpy() @ W.double().numpy().T + b.double().numpy()
    ref = np.cos(np.tanh(z64)) * np.sqrt(2.0 / F)
    with torch.no_grad():
        y32 = torch.cos(torch.tanh(torch.nn.functional.linear(x, W, b))) * np.sqrt(2.0 / F)
    yard = np.abs(y32.double().numpy() - ref).max()
    err = np.abs(phi - ref).max()
    print(f"[{case[0]}] rows {rows} K {K}: phi err {err:.2e}, fp32 yardstick {yard:.2e}")
    assert err <= 4 * yard
    valid = np.arange(rows) < n_valid
    if masked:
        valid &= mask.numpy() > 0
    want = (phi * valid[:, None]).reshape(rows // 32, 32, F).sum(1)
    np.testing.assert_allclose(part, want, rtol=1e-13, atol=0)


# ---- run.py's shape once ----------------------------------------------------------------------
def test_run_py_shape():
    """D 394 (S 197, 'ss'), hidden_dims [512] * 4, F 512 -- the net both run.py branches build --
    on 512 expert and 384 policy rows."""
    import amp_extensions_amd as amx
    S, A, F = 197, 36, 512
    es, ea, es2 = M.synthetic_rows(512, 3, S, A)
    ps, pa, ps2 = M.synthetic_rows(384, 4, S, A, shift=0.3)
    expert, x_pi = M.cost_rows("ss", es, ea, es2), M.cost_rows("ss", ps, pa, ps2)
    cost = amx.MLPCost(expert, hidden_dims=[512] * 4, feature_dim=F, bw_samples=10000, lambda_b=0.1, seed=100)
    assert cost.map.Kp == 416 and cost.map.n_hidden == 4
    ref = M.Ref64({k: v.numpy() for k, v in cost.net.state_dict().items()}, expert, F, [-1.0, 0.0], 0.1)
    ref.fit_cost(x_pi)
    y = M.Yardstick(ref, expert, x_pi)
    check_cost_against_fp64(cost, ref, y, x_pi, "run.py shape")


# ---- the engine ---------------------------------------------------------------------------------
S_E, A_E, B_E, K_E = 226, 28, 100, 2
MLP_E = dict(hidden_dims=[64, 96], feature_dim=128, bw_samples=5000, lambda_b=0.1, seed=100)


@pytest.fixture(scope="module")
def engine_model():
    import amp_extensions_amd as amx
    ctx, ens = make_ensemble(amx, S_E, A_E, MLP_E["feature_dim"])
    es, ea, es2 = M.synthetic_rows(300, 3, S_E, A_E)
    table = M.synthetic_rows(128, 1, S_E, A_E)[0].double().numpy()
    pw, log_std = R.init_policy_weights(S_E, A_E, (32, 32), seed=100)
    return amx, ctx, ens, M.cost_rows("ss", es, ea, es2), table, pw, log_std


def _engine(engine_model):
    amx, ctx, ens, expert, table, pw, log_std = engine_model
    cost = amx.MLPCost(expert, ctx=ctx, **MLP_E)
    pol = amx.DevicePolicy(ctx, pw, log_std, seed=1)
    eng = amx.RolloutEngine(ens, table, lanes=B_E, policy=pol, cost=cost, seed=5, max_steps=K_E)
    eng.reset_all()
    return eng, cost


def test_engine_rollout_relabel_matches_fp64(engine_model):
    """RolloutEngine with an MLPCost, B 100 (padded to 128 lanes: the row mask matters), K 2:
    rollout(); relabel() against the fp64 restatement on the recorded [s, s'] rows."""
    amx, ctx, ens, expert, *_ = engine_model
    eng, cost = _engine(engine_model)
    assert eng.Bp == 128 and eng.row_mask is not None and eng.kc == cost.map.Kp
    eng.rollout()
    info = eng.relabel()
    torch.cuda.synchronize()
    D = 2 * S_E
    x = eng.cost_in[:K_E, :B_E, :D].reshape(-1, D).cpu()
    ss = torch.cat([eng.obs[:K_E].float(), eng.next_obs[:K_E].float()], -1).reshape(-1, D).cpu()
    assert torch.equal(x, ss) and not eng.cost_in[:K_E, :B_E, D:].any()
    ref = M.Ref64({k: v.numpy() for k, v in cost.net.state_dict().items()}, expert, MLP_E["feature_dim"],
                  [-1.0, 0.0], MLP_E["lambda_b"])
    mmd = ref.fit_cost(x)
    y = M.Yardstick(ref, expert, x)
    phi = f64(eng.phi[:K_E, :B_E]).reshape(-1, MLP_E["feature_dim"])
    e_phi, e_w = np.abs(phi - ref.rep(x)).max(), np.abs(f64(cost.w) - ref.w).max()
    print(f"[engine] phi err {e_phi:.2e} (yardstick {y.phi_err:.2e})  w err {e_w:.2e} ({y.w_err:.2e})")
    assert e_phi <= y.d_phi and e_w <= y.d_w
    assert abs(float(info["mb_mmd"]) - mmd) <= M.mmd_bound(ref.w, y.d_w)
    disc = f64(eng.disc[:K_E, :B_E]).reshape(-1)
    c64, ipm64, wb64 = ref.bonus_costs(x, disc, ens.threshold)
    row = M.dot_bound(ref.rep(x), ref.w, y.d_phi, y.d_w)
    lam, slack = ref.lam, M.ulp4(ipm64, wb64)
    take = lambda t: f64(t[:K_E, :B_E]).reshape(-1)
    assert (np.abs(take(eng.ipm) - ipm64) <= (1 - lam) * row + slack).all()
    assert (np.abs(take(eng.wbonus) - wb64) <= slack).all()
    assert (np.abs(take(eng.rewards) + c64) <= (1 - lam) * row + slack).all()
    erow = M.dot_bound(ref.expert_rep, ref.w, y.d_phi, y.d_w)
    assert abs(float(cost.get_expert_cost()) - ref.expert_cost()) <= (1 - lam) * erow.mean() + M.ulp4(ref.expert_cost())


def test_engine_graph_replay_is_bit_identical(engine_model):
    """graph_rollout captures MlpMap.features (no allocation or synchronisation after the first
    call at a row count): three replays equal the same rollouts launched eagerly, bit for bit."""
    runs = []
    for graph in (False, True):
        eng, cost = _engine(engine_model)
        eng.rollout()
        eng.relabel()
        out = []
        replay = eng.graph_rollout(K_E, tail=cost.get_expert_cost) if graph else None
        for _ in range(3):
            if graph:
                replay()
            else:
                eng.rollout()
                eng.relabel()
                cost.get_expert_cost()
            out.append([t.clone() for t in (eng.obs, eng.acts, eng.phi, eng.rewards, eng.ipm, eng.mb_mmd,
                                            cost._expert_mean)])
        torch.cuda.synchronize()
        runs.append(out)
    for ea, eb in zip(*runs):
        for xa, xb in zip(ea, eb):
            assert torch.equal(xa, xb)
    assert not torch.equal(runs[1][0][1], runs[1][1][1])  # successive replays draw fresh noise


def test_relabel_paths_on_sampled_paths(engine_model):
    """relabel_paths (batch_reinforce.py:103-169) with an MLPCost on sample_points' paths: rewards
    and mb_mmd against the fp64 restatement."""
    amx, ctx, ens, expert, table, pw, log_std = engine_model
    from amp_extensions_amd.costs import device_discrepancy
    from amp_extensions_amd.relabel import relabel_paths
    cost = amx.MLPCost(expert, ctx=ctx, **MLP_E)
    pol = amx.DevicePolicy(ctx, pw, log_std)
    env = amx.BatchedSimEnv(ens, table, lanes=12, horizon=15, max_steps=8, record_means=True)
    paths = amx.sample_points(env, pol, num_to_collect=120, base_seed=1)
    rows = lambda k: torch.from_numpy(np.concatenate([p[k] for p in paths])).float()
    obs, act, nxt = rows("observations"), rows("actions"), rows("next_observations")
    infos = relabel_paths(paths, cost, ens)
    x = torch.cat([obs, nxt], 1)
    ref = M.Ref64({k: v.numpy() for k, v in cost.net.state_dict().items()}, expert, MLP_E["feature_dim"],
                  [-1.0, 0.0], MLP_E["lambda_b"])
    mmd = ref.fit_cost(x)
    y = M.Yardstick(ref, expert, x)
    assert abs(infos["mb_mmd"] - mmd) <= M.mmd_bound(ref.w, y.d_w)
    disc = f64(device_discrepancy(ens, obs.to(DEV), act.to(DEV)))
    c64, ipm64, wb64 = ref.bonus_costs(x, disc, ens.threshold)
    row = M.dot_bound(ref.rep(x), ref.w, y.d_phi, y.d_w)
    got = np.concatenate([p["rewards"] for p in paths]).astype(np.float64)
    assert (np.abs(got + c64) <= (1 - ref.lam) * row + M.ulp4(ipm64, wb64)).all()
    assert infos["ep_len"] == [len(p["observations"]) for p in paths] and np.isfinite(infos["bonus_mmd"])


# ---- shard_expert in one process ----------------------------------------------------------------
class _Done:
    def wait(self):
        pass


def test_shard_expert_partial_sums_reproduce_the_expert_cost():
    """Two ranks' partial expert sums, fed through a fake all-reduce (each rank's buffer receives
    the other's recorded partial), reproduce the unsharded expert cost."""
    import amp_extensions_amd as amx
    S, A = 24, 6
    es, ea, es2 = M.synthetic_rows(301, 3, S, A)     # an odd count: unequal blocks
    ps, pa, ps2 = M.synthetic_rows(200, 4, S, A, shift=0.3)
    expert, x_pi = M.cost_rows("ss", es, ea, es2), M.cost_rows("ss", ps, pa, ps2)
    ctx = amx.AmxContext(S, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=128, device=DEV)
    mk = lambda: amx.MLPCost(expert, hidden_dims=[64, 96, 64], feature_dim=128, bw_samples=5000, lambda_b=0.1,
                             seed=100, ctx=ctx)
    whole = mk()
    whole.fit_cost(x_pi)
    want = float(whole.get_expert_cost())
    parts = {}

    def fake(rank):
        def allreduce_async(buf):
            parts[rank] = buf.clone()
            if 1 - rank in parts:
                buf.add_(parts[1 - rank])
            return _Done()
        return allreduce_async

    ranks = [mk(), mk()]
    for r, c in enumerate(ranks):
        c.shard_expert(r, 2, fake(r))
        assert c.expert_sharded
    got = {}
    for r in (0, 1, 0):   # rank 0 again once rank 1's partial is known (fit_cost: a new w, a new sum)
        ranks[r].fit_cost(x_pi)
        got[r] = float(ranks[r].get_expert_cost())
    assert got[0] == got[1]
    torch.cuda.synchronize()
    total = float((parts[0] + parts[1]).item())
    # against fp64 sums of the device's own features: the kernel's per-row dot is fp32 (F + 2
    # roundings of 2^-24 on sum |phi_i w_i|), the sum over rows fp64
    rep, w = f64(whole.expert_rep), f64(whole.w)
    rows64 = np.clip(rep @ w, -1.0, 0.0)
    dot_err = (np.abs(rep) @ np.abs(w)) * (rep.shape[1] + 2) * 2.0 ** -24
    assert abs(total - rows64.sum()) <= dot_err.sum()
    lo, hi = ranks[0]._elo, ranks[0]._ehi
    assert (lo, hi) == (0, 151) and (ranks[1]._elo, ranks[1]._ehi) == (151, 301)
    assert abs(float(parts[0].item()) - rows64[lo:hi].sum()) <= dot_err[lo:hi].sum()
    assert abs(got[0] - want) <= float(np.spacing(np.float32(abs(want))))


# ---- checkpoint -----------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    """save_checkpoint's MLPCost entries (milo/utils.py:32-37: 'w' and 'net') through torch.save /
    torch.load, and back into a fresh net."""
    import amp_extensions_amd as amx
    from amp_extensions_amd.costs import mlp_cost_net
    S, A = 24, 6
    es, ea, es2 = M.synthetic_rows(300, 3, S, A)
    ps, pa, ps2 = M.synthetic_rows(200, 4, S, A, shift=0.3)
    cost = amx.MLPCost(M.cost_rows("ss", es, ea, es2), hidden_dims=[64, 96, 64], feature_dim=128, bw_samples=5000,
                       seed=100)
    cost.fit_cost(M.cost_rows("ss", ps, pa, ps2))
    path = str(tmp_path / "checkpoint_0.pt")
    torch.save({"w": cost.w, "net": cost.net.state_dict()}, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert torch.equal(ck["w"], cost.w.cpu()) and ck["w"].shape == (128,)
    assert list(ck["net"]) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias"]
    net = mlp_cost_net(2 * S, [64, 96, 64], 128)
    net.load_state_dict(ck["net"])
    for k, v in cost.net.state_dict().items():
        assert torch.equal(net.state_dict()[k], v)
