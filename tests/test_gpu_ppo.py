"""GPU parity of the device PPO update (amx_ppo_steps / amx_ppo_old_ll; DevicePPO, PPO) against
the reference's PPO.train_from_paths (mjrl/mjrl/algos/ppo_clip.py:58-121).

The comparator is tests/ppo_ref.py: the reference loop restated in torch on the CPU, run in fp64
(the yardstick) and in fp32 (the reference's own arithmetic; bit-identical to it on G20,
test_cpu_ppo.py).  Every comparison is test_gpu_bcfit.py's `check`: first fp32 alone within a
quarter of the tolerance of fp64, then the device within the tolerance of fp64.

Tolerances: 2e-5 * max(1, max|ref|) for theta, 1e-4 * max|ref| per tensor for exp_avg /
exp_avg_sq, 1e-4 relative for the step losses, 1e-3 relative for surr_after (test_gpu_npg.py's)
and 1e-3 |ref| + 1e-6 for kl_dist (at kl = 4.6e-5 its fp32 noise alone is 3e-3 relative).

The clipped surrogate has kinks at LR = 1 -/+ c: a row that two arithmetics put on different
sides gets a different gradient.  So every case first asserts, as conditions on the inputs, that
the fp32 and fp64 runs clip the same number of rows at every step and that no fp64 ratio is
closer than 2e-4 to a kink; the device's per-step counts must then equal the comparator's.
"""
import functools

import numpy as np
import pytest
import torch

import ppo_ref as R
from test_gpu_bcfit import NAMES, TOL_S, _MjrlMLP, check, check_adam, check_theta, optimizer_state

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOL_SURR = lambda ref: 1e-3 * float(np.max(np.abs(ref)))        # noqa: E731
TOL_KL = lambda ref: 1e-3 * float(np.max(np.abs(ref))) + 1e-6   # noqa: E731

CASES = {
    #  name             S    A   lens               epochs  lr    numpy seed
    "one_step": (197, 36, (64,), 1, 3e-4, 77),
    "ragged_default": (197, 36, (70, 130, 3, 120), 2, 3e-4, 77),
    "ragged_clipped": (197, 36, (70, 130, 3, 120), 2, 3e-3, 84),
    "other": (226, 28, (100, 28), 3, 3e-3, 77),
}


@functools.lru_cache(maxsize=None)
def inputs(name, calls=1):
    """(flat theta, obs, act, adv, [batches per call]) of a case: the issue's seeds."""
    from amp_extensions_amd.bc import plan_bc_batches
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    S, A, lens, epochs, _, seed = CASES[name]
    flat = pack_policy(*init_mlp_policy_params(S, A, seed=123, init_log_std=-0.25))
    obs, act, adv = R.concat(R.make_paths(lens, S, A, flat, seed=5))
    np.random.seed(seed)
    return flat, obs, act, adv, [plan_bc_batches(len(obs), epochs) for _ in range(calls)]


@functools.lru_cache(maxsize=None)
def reference(name, olds=("snapshot",), min_log_std=-3.0):
    """Per dtype (fp32, fp64): the outputs of the consecutive calls `olds`, with the flat
    parameters and the Adam state after each."""
    S, A, _, _, lr, _ = CASES[name]
    flat, obs, act, adv, batches = inputs(name, len(olds))
    res = []
    for dtype in (torch.float32, torch.float64):
        h = R.Host(flat, S, A, dtype, lr=lr, min_log_std=min_log_std)
        calls = []
        for old, b in zip(olds, batches):
            out = h.update(obs, act, adv, b, old=old)
            out["flat"] = h.flat()
            out["adam"] = tuple(x if isinstance(x, int) else [t.copy() for t in x] for x in h.adam())
            calls.append(out)
        res.append(calls)
    return res


def check_conditions(r32, r64, min_clipped_frac=0.0):
    """The inputs do not sit on a kink of the clipped surrogate."""
    assert np.array_equal(r32["step_clipped"], r64["step_clipped"])
    assert r64["margin"] >= 2e-4, r64["margin"]
    uses = 64 * len(r64["step_clipped"])
    print(f"clipped {int(r64['step_clipped'].sum())}/{uses}  margin {r64['margin']:.3g}")
    assert r64["step_clipped"].sum() >= min_clipped_frac * uses


def check_call(d, out, r32, r64, S, A):
    check("step losses", d.step_losses, r32["step_losses"], r64["step_losses"], TOL_S)
    assert np.array_equal(d.step_clipped, r64["step_clipped"])
    check("surr_after", out["surr_after"], r32["surr_after"], r64["surr_after"], TOL_SURR)
    check("kl_dist", out["kl_dist"], r32["kl_dist"], r64["kl_dist"], TOL_KL)
    check_adam(d.adam_state(), r32["adam"], r64["adam"], r64["adam"][0])


@pytest.fixture(scope="module")
def amx():
    import amp_extensions_amd as amx
    return amx


@pytest.fixture(scope="module")
def ctxs(amx):
    return {S: amx.AmxContext(S, A, n_models=1, hidden=16, n_hidden=1, feat_dim=256, device=DEV)
            for S, A in ((197, 36), (226, 28))}


def make_device(amx, ctxs, name, **kw):
    from amp_extensions_amd.npg import unpack_policy
    S, A, _, epochs, lr, _ = CASES[name]
    layers, log_std = unpack_policy(inputs(name)[0], S, A)
    return amx.DevicePPO(ctxs[S], layers, log_std, epochs=epochs, learn_rate=lr, **kw)


def device_call(amx, ctxs, name, **kw):
    _, obs, act, adv, batches = inputs(name)
    d = make_device(amx, ctxs, name)
    out = d.train_from_arrays(obs, act, adv, batches=batches[0], **kw)
    torch.cuda.synchronize()
    return d, out


# ---- tests -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_comparator(amx, ctxs, name):
    """Snapshot mode, one call: theta, the moments of all seven tensors, the step losses,
    surr_after and kl_dist; the per-step clipped counts exactly."""
    S, A = CASES[name][:2]
    (r32,), (r64,) = reference(name)
    check_conditions(r32, r64, 0.25 if name in ("ragged_clipped", "other") else 0.0)
    d, out = device_call(amx, ctxs, name)
    check_call(d, out, r32, r64, S, A)
    check_theta(d.get_param_values(), r32["flat"], r64["flat"], S, A)
    check("whitened advantages", out["advantages"].cpu().numpy(), r64["adv_w"], r64["adv_w"], lambda ref: 1e-12)
    # LR = exp(0) up to the EVAL pass's fp32 rounding of LL_new - LL_old
    assert abs(out["surr_before"] - r64["surr_before"]) <= 1e-6


def test_one_step(amx, ctxs):
    """N = 64, one step from a fresh state: the old policy is the new one, so LR == 1 exactly
    (amx_ppo_old_ll and the step share their arithmetic): nothing is clipped and the loss is
    -mean(adv) of the batch; g = adv reaches all seven tensors."""
    flat, _, _, _, batches = inputs("one_step")
    (r32,), (r64,) = reference("one_step")
    d, _ = device_call(amx, ctxs, "one_step")
    assert d.step_clipped.tolist() == [0] and r64["step_clipped"].tolist() == [0]
    adv32 = r64["adv_w"].astype(np.float32)[batches[0].reshape(-1)]
    assert abs(float(d.step_losses[0]) + float(np.mean(adv32.astype(np.float64)))) <= 1e-6
    step, m, v = d.adam_state()
    assert step == 1
    for n, a, b, mm in zip(NAMES, R.split_flat(flat, 197, 36), R.split_flat(d.get_param_values(), 197, 36), m):
        assert np.any(a != b), n
        assert mm.abs().max() > 0, n


@pytest.mark.parametrize("second", ["tracks_mean", "snapshot"])
def test_two_calls_and_the_old_policy(amx, ctxs, second):
    """ragged_clipped with min_log_std = -0.26, two calls; the second with the old mean network
    tracking the new one (what the reference computes: the write-back clamps 7 and then 14
    log_std entries) or as a snapshot again (PPO as written: there it clips 293 of 640 row uses
    and clamps 7 and then 12).  theta and the moments after each call."""
    name, S, A = "ragged_clipped", 197, 36
    olds = ("snapshot", second)
    r32, r64 = reference(name, olds, -0.26)
    _, obs, act, adv, batches = inputs(name, 2)
    d = make_device(amx, ctxs, name, min_log_std=-0.26, old="snapshot")
    clamped = []
    for c, old in enumerate(olds):
        check_conditions(r32[c], r64[c])
        d.old = old
        out = d.train_from_arrays(obs, act, adv, batches=batches[c])
        check_call(d, out, r32[c], r64[c], S, A)
        theta = d.get_param_values()
        check_theta(theta, r32[c]["flat"], r64[c]["flat"], S, A)
        clamped.append(int(np.sum(theta[-A:] == np.float32(-0.26))))
        assert theta[-A:].min() >= np.float32(-0.26) and torch.equal(d.theta, d.theta_old)
    assert clamped == [r64[c]["clamped"] for c in range(2)] == ([7, 14] if second == "tracks_mean" else [7, 12])
    if second == "snapshot":
        assert int(r64[1]["step_clipped"].sum()) == 293 and r64[1]["margin"] >= 1e-3


@pytest.mark.parametrize("k", ["default", "clipped"])
def test_g20_two_reference_calls_through_the_drop_in(amx, ctxs, golden, k):
    """The reference's PPO.train_from_paths called twice on one PPO object reproduces through
    the drop-in on a policy with mjrl MLP's layout and write-back: before the second call
    old_model's tensors share model's storage, and the drop-in switches form by itself."""
    g = golden("g20_ppo_update.npz")
    S, A, lens = 197, 36, [int(l) for l in g["lens"]]
    lr, mls = float(g[f"{k}_learn_rate"]), float(g[f"{k}_min_log_std"])
    pol = _MjrlMLP(S, A, seed=int(g["model_seed"]), min_log_std=mls)
    flat0 = pol.get_param_values()
    paths = R.make_paths(lens, S, A, flat0, seed=int(g["path_seed"]))
    obs, act, adv = R.concat(paths)

    np.random.seed(int(g[f"{k}_numpy_seed"]))
    h64 = R.Host(flat0, S, A, torch.float64, lr=lr, min_log_std=mls)
    r64, flat64 = [], []
    for old in ("snapshot", "tracks_mean"):
        r64.append(h64.update(obs, act, adv, amx.plan_bc_batches(len(obs), 2), old=old))
        flat64.append(h64.flat())

    ppo = amx.PPO(None, pol, None, epochs=2, mb_size=64, learn_rate=lr, save_logs=True, ctx=ctxs[S])
    np.random.seed(int(g[f"{k}_numpy_seed"]))
    modes = []
    for c in range(2):
        stats = ppo.train_from_paths(paths)
        modes.append(ppo.device_ppo.old)
        check_theta(pol.get_param_values(), g[f"{k}_params_{c}"], flat64[c], S, A)
        assert np.array_equal(np.array(stats, dtype=np.float64), g[f"{k}_base_stats"])
    assert modes == ["snapshot", "tracks_mean"]
    assert ppo.running_score == float(g[f"{k}_running_score"])
    ref32 = (int(g[f"{k}_step"]), [g[f"{k}_exp_avg_{i}"] for i in range(7)], [g[f"{k}_exp_avg_sq_{i}"] for i in range(7)])
    assert len(ppo.optimizer.state) == 7
    check_adam(optimizer_state(ppo.optimizer, pol.trainable_params), ref32, h64.adam(), 20)
    log = ppo.logger.log
    assert len(log["t_opt"]) == 2 and len(log["running_score"]) == 2
    for c in range(2):
        check(f"kl_dist {c}", log["kl_dist"][c], g[f"{k}_kl_dist"][c], r64[c]["kl_dist"], TOL_KL)
        check(f"surr_improvement {c}", log["surr_improvement"][c], g[f"{k}_surr_improvement"][c],
              r64[c]["surr_after"] - r64[c]["surr_before"], TOL_SURR)


def abi_run(ctxs, name, cuts):
    """amx_ppo_old_ll and amx_ppo_steps in launches of `cuts` steps -> (theta, m, v, step,
    losses, clipped)."""
    from amp_extensions_amd import _native as N
    S = CASES[name][0]
    lr = CASES[name][4]
    flat, obs, act, adv, batches = inputs(name)
    c = ctxs[S]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(DEV)  # noqa: E731
    obs, act, adv = t(obs, torch.float32), t(act, torch.float32), t(R.whiten(adv), torch.float32)
    idx = t(batches[0].reshape(-1, 64), torch.int32)
    n, total = obs.shape[0], idx.shape[0]
    assert sum(cuts) == total
    theta = t(flat, torch.float32)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    ll = torch.empty(n, dtype=torch.float32, device=DEV)
    losses = torch.zeros(total, dtype=torch.float32, device=DEV)
    clipped = torch.zeros(total, dtype=torch.int32, device=DEV)
    N.check(c.lib.amx_ppo_old_ll(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                 theta.data_ptr(), ll.data_ptr(), c.stream), "amx_ppo_old_ll")
    k0 = 0
    for k in cuts:
        N.check(c.lib.amx_ppo_steps(c.h, n, obs.data_ptr(), obs.stride(0), act.data_ptr(), act.stride(0),
                                    adv.data_ptr(), ll.data_ptr(), None, N.AMX_PPO_OLD_SNAPSHOT, idx[k0:].data_ptr(), k,
                                    theta.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr, 0.9, 0.999,
                                    1e-8, 0.2, losses[k0:].data_ptr(), clipped[k0:].data_ptr(), c.stream),
                "amx_ppo_steps")
        k0 += k
    torch.cuda.synchronize()
    return theta, m, v, step, losses, clipped


def test_launch_cut_changes_no_bit_and_runs_repeat(amx, ctxs):
    """ragged_clipped's 10 steps in one launch, in launches of 3, 3 and 4, and once more in one:
    theta, the moments, the losses and the counts are identical; DevicePPO's own cut as well."""
    one, cut, again = (abi_run(ctxs, "ragged_clipped", c) for c in ((10,), (3, 3, 4), (10,)))
    for a, b, e in zip(one, cut, again):
        assert torch.equal(a, b) and torch.equal(a, e)
    assert int(one[3].item()) == 10 and int(one[5].sum().item()) > 160
    d1, o1 = device_call(amx, ctxs, "ragged_clipped")
    d2, o2 = device_call(amx, ctxs, "ragged_clipped", max_steps_per_launch=3)
    assert torch.equal(d1.theta, d2.theta) and all(torch.equal(x, y) for x, y in zip(d1._bc._adam, d2._bc._adam))
    assert np.array_equal(d1.step_losses, d2.step_losses) and np.array_equal(d1.step_clipped, d2.step_clipped)
    assert {k: v for k, v in o1.items() if k != "advantages"} == {k: v for k, v in o2.items() if k != "advantages"}
    # the engine object runs the entry points as abi_run does (host-whitened advantages there)
    assert np.array_equal(d1.step_clipped, one[5].cpu().numpy())


def test_optimizer_round_trip_and_resume(amx, ctxs):
    """adam_state -> a torch Adam -> load_optimizer gives the same state back; a fresh PPO on the
    same policy with the first object's optimizer continues to the same parameters as one
    object called twice, bit for bit."""
    S, A, lens, epochs, lr, seed = CASES["ragged_clipped"]
    flat0 = inputs("ragged_clipped")[0]
    paths = R.make_paths(lens, S, A, flat0, seed=5)
    thetas = []
    for fresh in (False, True):
        pol = _MjrlMLP(S, A, seed=123, min_log_std=-0.26)
        ppo = amx.PPO(None, pol, None, epochs=epochs, learn_rate=lr, ctx=ctxs[S])
        np.random.seed(seed)
        ppo.train_from_paths(paths)
        if fresh:
            first = ppo
            ppo = amx.PPO(None, pol, None, epochs=epochs, learn_rate=lr, ctx=ctxs[S])
            ppo.optimizer = first.optimizer
        ppo.train_from_paths(paths)
        assert optimizer_state(ppo.optimizer, pol.trainable_params)[0] == 20
        thetas.append(pol.get_param_values())
    assert np.array_equal(thetas[0], thetas[1])

    d = make_device(amx, ctxs, "ragged_clipped")
    d.load_optimizer(ppo.optimizer)
    step, m, v = d.adam_state()
    ref = optimizer_state(ppo.optimizer, pol.trainable_params)
    assert step == 20 and all(np.array_equal(a.numpy(), b) for a, b in zip(m, ref[1]))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(v, ref[2]))


def test_refusals(amx, ctxs):
    """Unsupported configurations raise before anything is launched: no device object exists
    afterwards and the policy and the optimizer are untouched."""
    S, A = 197, 36
    flat0 = inputs("one_step")[0]
    paths = R.make_paths((64,), S, A, flat0, seed=5)

    def built(exc, hidden=(32, 32), transform=False, **kw):
        pol = _MjrlMLP(S, A, hidden=hidden, seed=123)
        if transform:
            pol.model.transformations["in_shift"] = np.zeros(S)
        before = pol.get_param_values()
        made = []
        with pytest.raises(exc):
            made.append(amx.PPO(None, pol, None, ctx=ctxs[S], **kw))
        assert not made and np.array_equal(pol.get_param_values(), before)

    built(NotImplementedError, hidden=(64, 64))
    built(NotImplementedError, mb_size=32)
    built(NotImplementedError, transform=True)

    def trained(opt=None, share_one=False):
        pol = _MjrlMLP(S, A, seed=123)
        ppo = amx.PPO(None, pol, None, ctx=ctxs[S])
        if opt:
            ppo.optimizer = opt(pol.trainable_params)
        if share_one:
            pol.old_model.fc_layers[0].weight.data = pol.model.fc_layers[0].weight.data
        before = pol.get_param_values()
        with pytest.raises(NotImplementedError):
            ppo.train_from_paths(paths)
        assert ppo.device_ppo is None and np.array_equal(pol.get_param_values(), before)
        assert not ppo.optimizer.state and ppo.running_score is None and ppo.logger.log == {}

    trained(opt=lambda p: torch.optim.SGD(p, lr=1e-3))
    trained(opt=lambda p: torch.optim.Adam(p, lr=1e-3, amsgrad=True))
    trained(share_one=True)
    with pytest.raises(ValueError):
        make_device(amx, ctxs, "one_step", old="frozen")
    with pytest.raises(NotImplementedError):
        make_device(amx, ctxs, "one_step", mb_size=128)


def test_train_from_engine_is_train_from_arrays(amx):
    """On the rollout engine's buffers (test_gpu_npg.py's smallest engine: 4 steps of 256 lanes)
    the update equals train_from_arrays on the same rows bit for bit and refreshes the sampler's
    policy."""
    from amp_extensions_amd import synthetic as syn
    from amp_extensions_amd.ensemble import init_ensemble_weights
    from amp_extensions_amd.policy import init_mlp_policy_params
    import oracle.milo_ref as M
    S, A = 197, 36
    s, a, s2 = syn.offline(2048, S, A, 0)
    norms = M.get_transformations(*[torch.from_numpy(x).float() for x in (s, a, s2)])
    ctx = amx.AmxContext(S, A, n_models=4, hidden=128, n_hidden=2, device=DEV)
    ens = amx.DeviceEnsemble(ctx, init_ensemble_weights(S, A, [128] * 2, 4, 100), norms)
    layers, ls = init_mlp_policy_params(S, A)
    pol = amx.DevicePolicy(ctx, layers, ls, seed=3)
    eng = amx.RolloutEngine(ens, syn.reset_table(512, S, 1), lanes=256, policy=pol, seed=5, max_steps=4)
    eng.reset_all()
    eng.rollout()
    T, B = eng.t, eng.B
    adv = torch.randn(T, B, dtype=torch.float64, device=DEV)
    np.random.seed(3)
    batches = amx.plan_bc_batches(T * B, 1)
    blob0 = pol.blob.clone()
    a_ = amx.DevicePPO(ctx, layers, ls, epochs=1, learn_rate=3e-3, policy=pol)
    out_a = a_.train_from_engine(eng, adv, batches=batches)
    assert not torch.equal(blob0, pol.blob)
    b_ = amx.DevicePPO(ctx, layers, ls, epochs=1, learn_rate=3e-3)
    out_b = b_.train_from_arrays(eng.obs[:T].reshape(T * B, S), eng.acts[:T].reshape(T * B, A), adv.reshape(-1),
                                 batches=batches)
    from amp_extensions_amd.npg import pack_policy
    assert torch.equal(a_.theta, b_.theta)
    assert not np.array_equal(a_.get_param_values(), pack_policy(layers, ls))
    assert np.array_equal(a_.step_losses, b_.step_losses) and len(a_.step_losses) == T * B // 64
    assert all(out_a[k] == out_b[k] for k in ("surr_before", "surr_after", "kl_dist"))
    assert out_a["kl_dist"] > 0
