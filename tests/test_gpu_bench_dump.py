"""bench.py --dump-outputs: the arrays of the last rollout as .npy files.  A small engine
(1500 lanes x 3 steps = 4500 transitions: more than DUMP_SAMPLE_ROWS, so the wide rows are
sampled; 1500 lanes pad to 1536, so the padded lanes must be dropped) runs one rollout +
relabel, bench.dump_outputs writes it, and the files are compared with the engine's buffers."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
S, A, B, T = 197, 36, 1500, 3


@pytest.fixture(scope="module")
def rollout():
    import amp_extensions_amd as amx
    from amp_extensions_amd import synthetic as syn
    from amp_extensions_amd.datasets import get_transformations
    from amp_extensions_amd.ensemble import init_ensemble_weights
    from amp_extensions_amd.policy import init_mlp_policy_params
    s, a, s2 = syn.offline(4096, S, A, 0)
    st, at, s2t = (torch.from_numpy(x).float() for x in (s, a, s2))
    ctx = amx.AmxContext(S, A, n_models=4, hidden=512, n_hidden=4, feat_dim=512, device="cuda")
    ens = amx.DeviceEnsemble(ctx, init_ensemble_weights(S, A, [512] * 4, 4, base_seed=100),
                             get_transformations(st, at, s2t))
    ens.compute_threshold(st.cuda(), at.cuda())
    cost = amx.RBFLinearCost(torch.from_numpy(syn.expert(2048, S, 3)), feature_dim=512, bw_quantile=0.1,
                             bw_samples=4096, lambda_b=0.0025, seed=100, ctx=ctx)
    pw, log_std = init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25)
    eng = amx.RolloutEngine(ens, syn.reset_table(4096, S, 1), lanes=B, policy=amx.DevicePolicy(ctx, pw, log_std, seed=1),
                            cost=cost, seed=2, max_steps=T)
    eng.reset_all()
    eng.rollout(T)
    eng.relabel()
    last = {"expert_cost": cost.get_expert_cost()}
    torch.cuda.synchronize()
    return eng, cost, last


def _dump(rollout, out_dir):
    import bench
    eng, cost, last = rollout
    args = types.SimpleNamespace(mode="engine", cost="mmd")
    shapes = bench.dump_outputs(str(out_dir), args, eng, cost, T, last)
    files = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}
    assert set(files) == set(shapes) and all(list(files[k].shape) == shapes[k] for k in shapes)
    return bench, files


def test_dump_matches_the_engine_buffers(rollout, tmp_path):
    bench, f = _dump(rollout, tmp_path)
    eng, cost, last = rollout
    n = T * B
    assert all(a.dtype in (np.float32, np.float64) for a in f.values())
    assert sum(a.nbytes for a in f.values()) <= bench.DUMP_LIMIT_BYTES
    rows = f["sample_rows"].astype(np.int64)
    assert rows.shape == (bench.DUMP_SAMPLE_ROWS,) and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < n
    obs = eng.obs[:T].cpu().numpy().reshape(n, S)
    nxt = eng.next_obs[:T].cpu().numpy().reshape(n, S)
    act = eng.acts[:T].cpu().numpy().reshape(n, A)
    assert f["observations"].dtype == np.float64 and np.array_equal(f["observations"], obs[rows])
    assert np.array_equal(f["next_observations"], nxt[rows])
    assert np.array_equal(f["actions"], act[rows])
    # per-transition scalars whole, in (step, lane) order, without the padded lanes
    for name, buf in (("rewards", eng.rewards), ("ipm", eng.ipm), ("bonus", eng.wbonus), ("disagreement", eng.disc)):
        assert f[name].shape == (n,) and f[name].dtype == np.float32
        assert np.array_equal(f[name], buf[:T, :B].cpu().numpy().reshape(n)), name
    assert np.array_equal(f["done"], eng.done[:T].cpu().numpy().reshape(n).astype(np.float32))
    assert np.array_equal(f["feature_sum"], eng.phi_sum.cpu().numpy())
    assert f["mb_mmd"][0] == np.float32(eng.mb_mmd.item()) and f["expert_cost"][0] == np.float32(last["expert_cost"].item())
    assert all(np.isfinite(a).all() for a in f.values())
    assert np.abs(f["rewards"]).max() > 0 and np.abs(f["observations"]).max() > 0


def test_dump_is_repeatable(rollout, tmp_path):
    """The same state dumped twice gives the same files: the row sample is drawn from a fixed seed."""
    _, f1 = _dump(rollout, tmp_path / "a")
    _, f2 = _dump(rollout, tmp_path / "b")
    assert all(np.array_equal(f1[k], f2[k]) for k in f1)
