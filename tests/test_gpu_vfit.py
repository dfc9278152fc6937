"""GPU parity of the device value-baseline fit (amx_vfit_epoch; DeviceMLPBaseline.fit /
fit_grid / sync_to, RolloutEngine.fit_baseline) against the reference's MLPBaseline.fit.

The comparator is a restatement of the reference loop (mjrl/mjrl/utils/optimize_model.py:21-35
under mlp_baseline.py:61-97) in torch on the CPU: nn.Sequential of Linear / ReLU,
torch.optim.Adam(lr, weight_decay), MSELoss, injected permutations.  It runs twice, in fp64
(the yardstick) and in fp32 (the reference's own arithmetic).  Every comparison first asserts
that fp32 alone is within a quarter of the tolerance of fp64 (so the inputs do not sit on one
of Adam's lr * g / (|g| + eps) cliffs, where rounding noise in a near-zero gradient moves a
weight by up to lr), then that the device is within the tolerance of fp64.

Tolerances (DESIGN.md's table): 2e-5 * max(1, max|ref|) for weights and predictions (the
fp32 GEMM-order tolerance), 1e-4 relative for the scalars error_before / error_after /
epoch_losses and 1e-4 * max|ref| per tensor for exp_avg / exp_avg_sq (the reduction
tolerance).  G14 (tests/golden/make_golden_vfit.py) is the reference's own two consecutive
fits; there the recorded fp32 results take the place of the fp32 restatement.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import milo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, REG = 1e-3, 1e-3


# ---- the reference loop, restated ------------------------------------------------------------

class Host:
    """What the device baseline mirrors: `.model`, `.optimizer`, batch_size, epochs."""

    def __init__(self, layers, dtype, lr=LR, reg=REG, epochs=1):
        mods = []
        for i, (W, b) in enumerate(layers):
            lin = nn.Linear(W.shape[1], W.shape[0]).to(dtype)
            with torch.no_grad():
                lin.weight.copy_(torch.as_tensor(W).to(dtype))
                lin.bias.copy_(torch.as_tensor(b).to(dtype))
            mods.append(lin)
            if i < len(layers) - 1:
                mods.append(nn.ReLU())
        self.model = nn.Sequential(*mods)
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, weight_decay=reg)
        self.loss = nn.MSELoss()
        self.dtype, self.batch_size, self.epochs = dtype, 64, epochs

    def predict(self, feat):
        with torch.no_grad():
            return self.model(torch.from_numpy(feat).to(self.dtype)).numpy().ravel()

    def fit(self, feat, returns, perms):
        """MLPBaseline.fit(return_errors=True, return_all_errors=True) on float32 features and
        returns, with fit_data's permutations injected."""
        x = torch.from_numpy(feat).to(self.dtype)
        y = torch.from_numpy(returns.astype(np.float32).reshape(-1, 1)).to(self.dtype)

        def error():
            e = y.numpy().ravel() - self.predict(feat)
            return np.sum(e ** 2) / (np.sum(y.numpy() ** 2) + 1e-8)

        before, losses = error(), []
        for perm in perms:
            idx = torch.as_tensor(np.asarray(perm), dtype=torch.long)
            num_steps = int(x.shape[0] / 64) - 1
            ep = 0.0
            for mb in range(num_steps):
                i = idx[mb * 64:(mb + 1) * 64]
                self.optimizer.zero_grad()
                loss = self.loss(self.model(x[i]), y[i])
                loss.backward()
                self.optimizer.step()
                ep = ep + loss.detach()
            losses.append(ep.numpy().ravel() / num_steps)
        return before, error(), losses

    def layers(self):
        return [(m.weight.detach().numpy(), m.bias.detach().numpy()) for m in self.model if isinstance(m, nn.Linear)]

    def adam(self):
        ps = self.optimizer.param_groups[0]["params"]
        st = [self.optimizer.state[p] for p in ps]
        return int(st[0]["step"]), [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st]


def make_paths(seed, lens, S):
    rs = np.random.RandomState(seed)
    paths = []
    for l in lens:
        obs = rs.randn(l, S) * 4.0
        obs[:, 3] *= 6.0  # some |x| > 10: the clip is live
        paths.append(dict(observations=obs, rewards=np.zeros(l, dtype=np.float32), returns=rs.randn(l) * 2.0 + 1.0))
    return paths


def returns_of(paths):
    return np.concatenate([p["returns"] for p in paths]).astype(np.float32)


# ---- comparisons -----------------------------------------------------------------------------

TOL_W = lambda ref: 2e-5 * max(1.0, float(np.max(np.abs(ref))))  # noqa: E731  weights, predictions
TOL_S = lambda ref: 1e-4 * float(np.max(np.abs(ref)))            # noqa: E731  scalars (relative)
TOL_M = lambda ref: 1e-4 * float(np.max(np.abs(ref)))            # noqa: E731  moments, per tensor


def check(what, dev, ref32, ref64, tol_fn):
    dev, ref32, ref64 = (np.asarray(a, dtype=np.float64) for a in (dev, ref32, ref64))
    assert dev.shape == ref64.shape == ref32.shape, what
    tol = tol_fn(ref64)
    own, gap = float(np.max(np.abs(ref32 - ref64))), float(np.max(np.abs(dev - ref64)))
    print(f"{what}: fp32-vs-fp64 {own:.3g}  device-vs-fp64 {gap:.3g}  tol {tol:.3g}")
    assert own <= tol / 4, f"{what}: the reference's own fp32 error {own:.3g} exceeds tol/4 = {tol / 4:.3g}"
    assert gap <= tol, f"{what}: device gap {gap:.3g} exceeds {tol:.3g}"


def check_state(bl, h32, h64, steps):
    names = ["W0", "b0", "W1", "b1", "W2", "b2"]
    flat = lambda ls: [a for Wb in ls for a in Wb]  # noqa: E731
    for n, d, a, b in zip(names, flat(bl.layers()), flat(h32.layers()), flat(h64.layers())):
        check(n, d.numpy().reshape(b.shape), a, b, TOL_W)
    step, m, v = bl.adam_state()
    s32, m32, v32 = h32.adam()
    s64, m64, v64 = h64.adam()
    assert step == s32 == s64 == steps
    for n, d, a, b in zip(names, m, m32, m64):
        check("exp_avg " + n, d.numpy().reshape(b.shape), a, b, TOL_M)
    for n, d, a, b in zip(names, v, v32, v64):
        check("exp_avg_sq " + n, d.numpy().reshape(b.shape), a, b, TOL_M)


def check_returns(out, r32, r64):
    for n, d, a, b in zip(("error_before", "error_after"), out[:2], r32[:2], r64[:2]):
        check(n, d, a, b, TOL_S)
    assert len(out[2]) == len(r64[2]) and all(l.shape == (1,) and l.dtype == np.float32 for l in out[2])
    check("epoch_losses", np.concatenate(out[2]), np.concatenate(r32[2]), np.concatenate(r64[2]), TOL_S)


def check_padding_is_zero(bl):
    """Everything outside the live blocks of the padded weights, biases and moments is exactly 0."""
    live, P = bl.layout.live_mask(), bl.layout.size
    flat_w = torch.cat([bl.W[0].reshape(-1), bl.b[0], bl.W[1].reshape(-1), bl.b[1], bl.w_head, bl.b_head]).cpu()
    assert flat_w.numel() == P and (~live).sum() > 0
    for name, t in (("weights", flat_w), ("exp_avg", bl._adam[0].cpu()), ("exp_avg_sq", bl._adam[1].cpu())):
        assert not t[~live].any(), f"padded {name} moved"
        assert t[live].any()


# ---- cases (host part cached: computed once per module) ---------------------------------------

CASES = {
    #  name         S    hidden      lens                     epochs  perm
    "one_step": (226, (128, 128), (128,), 1, "random"),
    "ragged": (226, (128, 128), (50, 100, 3, 180), 1, "random"),
    "three_paths": (226, (128, 128), (50, 100, 3, 180), 1, "three_paths"),
    "padding": (197, (64, 32), (200, 184), 1, "random"),
    "two_fits": (226, (128, 128), (90, 230), 1, "random"),
}


def case_perms(name, n, epochs, kind):
    rs = np.random.RandomState(sum(map(ord, name)))
    perms = [rs.permutation(n) for _ in range(epochs)]
    if kind == "three_paths":  # first batch: rows of paths 0, 1 and 2 (lens 50, 100, 3)
        first = np.concatenate([np.arange(30, 50), np.arange(150, 153), np.arange(50, 91)])
        rest = np.setdiff1d(np.arange(n), first)
        perms = [np.concatenate([first, rs.permutation(rest)])]
    return perms


@functools.lru_cache(maxsize=None)
def reference(name):
    """(layers, paths, feat, returns, perms, fp32 host, fp64 host, fp32 results, fp64 results) of a
    case after one fit; the two hosts keep their state for tests that go on."""
    S, hidden, lens, epochs, kind = CASES[name]
    layers = R.init_mlp_baseline(S, hidden, seed=11 + len(name))
    paths = make_paths(100 + len(name), lens, S)
    feat, y = R.mlp_baseline_features(paths), returns_of(paths)
    perms = case_perms(name, len(y), epochs, kind)
    h32, h64 = Host(layers, torch.float32, epochs=epochs), Host(layers, torch.float64, epochs=epochs)
    r32, r64 = h32.fit(feat, y, perms), h64.fit(feat, y, perms)
    return layers, paths, feat, y, perms, h32, h64, r32, r64


@pytest.fixture(scope="module")
def amx():
    import amp_extensions_amd as amx
    return amx


@pytest.fixture(scope="module")
def ctxs(amx):
    return {S: amx.AmxContext(S, A, n_models=4, hidden=64, n_hidden=4, feat_dim=128, device=DEV)
            for S, A in ((226, 28), (197, 36))}


def device_baseline(amx, ctxs, name, **kw):
    S, _, _, epochs, _ = CASES[name]
    return amx.DeviceMLPBaseline(ctxs[S], reference(name)[0], learn_rate=LR, reg_coef=REG, epochs=epochs, **kw)


def run_case(amx, ctxs, name):
    _, paths, _, _, perms, h32, h64, r32, r64 = reference(name)
    bl = device_baseline(amx, ctxs, name)
    out = bl.fit(paths, return_errors=True, return_all_errors=True, perms=perms)
    torch.cuda.synchronize()
    check_returns(out, r32, r64)
    check_state(bl, h32, h64, h64.adam()[0])
    return bl


# ---- tests -----------------------------------------------------------------------------------

def test_one_step_from_fresh_state(amx, ctxs):
    """N = 128: int(128 / 64) - 1 = 1 step.  Bias correction at t = 1, decay on the biases, the
    ReLU mask and the 2 / 64 factor all show in the weights and moments of this one step."""
    bl = run_case(amx, ctxs, "one_step")
    assert bl.adam_state()[0] == 1
    # without return_errors the reference returns None
    assert device_baseline(amx, ctxs, "one_step").fit(reference("one_step")[1], perms=reference("one_step")[4]) is None


@pytest.mark.parametrize("name", ["ragged", "three_paths"])
def test_ragged_rows_and_gather(amx, ctxs, name):
    """N = 333: 4 steps over 256 of the rows, 77 never touched; batches gather rows >= 256 and,
    in `three_paths`, rows of three different paths (their time features restart)."""
    perms = reference(name)[4]
    used = perms[0][:256]
    assert len(perms[0]) == 333 and used.max() >= 256
    if name == "three_paths":
        assert {int(np.searchsorted([50, 150, 153], i, side="right")) for i in used[:64]} == {0, 1, 2}
    bl = run_case(amx, ctxs, name)
    assert bl.adam_state()[0] == 4


def test_padding_stays_inert(amx, ctxs):
    """S = 197: kf = 224 with 201 live columns; hidden (64, 32) inside the 128-wide pads.  After
    5 steps the fit matches the restatement and no padded weight, bias or moment has moved."""
    bl = run_case(amx, ctxs, "padding")
    assert bl.kf == 224 and bl.Hp == [128, 128] and bl.adam_state()[0] == 5
    check_padding_is_zero(bl)


def g14_paths(seed, lens, S=226):
    """tests/golden/make_golden_vfit.py's g14_paths, restated (the fixture stores seeds, not inputs)."""
    rs = np.random.RandomState(seed)
    paths = []
    for l in lens:
        obs = rs.randn(l, S) * 4.0
        obs[:, 3] *= 6.0
        paths.append(dict(observations=obs, rewards=np.zeros(l, dtype=np.float32), returns=rs.randn(l) * 2.0 + 1.0))
    return paths


def test_g14_two_reference_fits(amx, ctxs, golden):
    """The reference's MLPBaseline.fit called twice (2 epochs of 5 steps each; the second call
    resumes Adam at step 10) reproduces: return values, final weights and optimizer state, with
    the permutations drawn from numpy's global RNG exactly as the reference consumed it."""
    g = golden("g14_baseline_fit.npz")
    lens = [int(l) for l in g["lens"]]
    n = sum(lens)
    layers = R.init_mlp_baseline(226, (128, 128), seed=int(g["model_seed"]))
    calls = [g14_paths(int(s), lens) for s in g["path_seeds"]]
    np.random.seed(int(g["numpy_seed"]))
    perms = [[np.random.permutation(n) for _ in range(2)] for _ in calls]
    h64 = Host(layers, torch.float64, epochs=2)
    r64 = [h64.fit(R.mlp_baseline_features(p), returns_of(p), pm) for p, pm in zip(calls, perms)]

    bl = amx.DeviceMLPBaseline(ctxs[226], layers, learn_rate=LR, reg_coef=REG, batch_size=64, epochs=2)
    np.random.seed(int(g["numpy_seed"]))
    outs = [bl.fit(p, return_errors=True, return_all_errors=True) for p in calls]
    torch.cuda.synchronize()
    for c, (out, r) in enumerate(zip(outs, r64)):
        r32 = (g[f"error_before_{c}"], g[f"error_after_{c}"], [l.reshape(1) for l in g[f"epoch_losses_{c}"]])
        check_returns(out, r32, r)
    keys = ["model.fc_0.weight", "model.fc_0.bias", "model.fc_1.weight", "model.fc_1.bias", "model.fc_2.weight",
            "model.fc_2.bias"]
    ref32 = types.SimpleNamespace(
        layers=lambda: [(g[keys[2 * i]], g[keys[2 * i + 1]]) for i in range(3)],
        adam=lambda: (int(g["step"]), [g[f"exp_avg_{i}"] for i in range(6)], [g[f"exp_avg_sq_{i}"] for i in range(6)]))
    check_state(bl, ref32, h64, 20)


def test_engine_layout(amx, ctxs):
    """RolloutEngine.fit_baseline over 128 lanes x 3 steps (384 rows, 5 steps): the rows, their
    order and the in-trajectory positions (t0 > 0 on lanes that continue a trajectory) are the
    ones advantages() uses, and advantages() afterwards predicts with the fitted weights."""
    from amp_extensions_amd import synthetic as syn
    from amp_extensions_amd.ensemble import init_ensemble_weights
    from amp_extensions_amd.policy import init_mlp_policy_params
    S, A, B, K = 197, 36, 128, 3
    ctx = ctxs[S]
    s, a, s2 = syn.offline(2048, S, A, 0)
    norms = R.get_transformations(*[torch.from_numpy(x).float() for x in (s, a, s2)])
    ens = amx.DeviceEnsemble(ctx, init_ensemble_weights(S, A, [64] * 4, 4, 100), norms)
    pw, ls = init_mlp_policy_params(S, A)
    pol = amx.DevicePolicy(ctx, pw, ls, seed=5)
    eng = amx.RolloutEngine(ens, syn.reset_table(4096, S, 1), lanes=B, term=amx.TerminationConfig(horizon=4),
                            policy=pol, seed=3, max_steps=K)
    eng.reset_all()
    eng.rollout(K)
    eng.rollout(K)  # second rollout: lanes start mid-trajectory
    eng.rewards.normal_(std=0.3)
    layers = R.init_mlp_baseline(S, (128, 128), seed=21)
    bl = amx.DeviceMLPBaseline(ctx, layers, learn_rate=LR, reg_coef=REG)
    adv0 = eng.advantages(bl)
    v0 = adv0["values"].clone()
    perm = np.random.RandomState(5).permutation(K * B)
    out = eng.fit_baseline(bl, adv0["returns"], perms=[perm], return_errors=True, return_all_errors=True)
    v1 = eng.advantages(bl)["values"]
    torch.cuda.synchronize()

    done, steps0 = eng.done[:K].cpu().numpy(), eng.steps0.cpu().numpy()
    assert steps0.max() > 0 and done.sum() > 0
    paths, rows = R.lanes_to_paths(done, eng.rewards[:K, :B].cpu().numpy(), eng.obs[:K].cpu().numpy(), steps0)
    feat_p = R.mlp_baseline_features(paths)
    feat = np.empty_like(feat_p)
    feat[np.concatenate([ts * B + b for ts, b in rows])] = feat_p  # path order -> row t * B + lane
    y = adv0["returns"].cpu().numpy().reshape(-1).astype(np.float32)
    h32, h64 = Host(layers, torch.float32), Host(layers, torch.float64)
    r32, r64 = h32.fit(feat, y, [perm]), h64.fit(feat, y, [perm])
    check_returns(out, r32, r64)
    check_state(bl, h32, h64, 5)
    check("values after the fit", v1.cpu().numpy().reshape(-1), h32.predict(feat), h64.predict(feat), TOL_W)
    assert float((v1 - v0).abs().max()) > 1e-3  # the fit moved the predictions


def test_fit_is_deterministic(amx, ctxs):
    _, paths, _, _, perms, *_ = reference("ragged")
    bls = [device_baseline(amx, ctxs, "ragged") for _ in range(2)]
    for bl in bls:
        bl.fit(paths, perms=perms)
    torch.cuda.synchronize()
    a, b = bls
    for x, y in zip(a.W + a.b + [a.w_head, a.b_head] + list(a._adam), b.W + b.b + [b.w_head, b.b_head] + list(b._adam)):
        assert torch.equal(x, y)


def test_sync_to_round_trip(amx, ctxs):
    """sync_to hands weights and Adam state to a host model + optimizer: it predicts what the
    device predicts, its state_dict carries the step count, and one more fit continued on the
    host matches the same fit continued on the device.  from_mjrl goes the other way."""
    layers, paths, feat, y, perms, h32, h64, _, _ = reference("two_fits")
    n = len(y)
    steps = int(n / 64) - 1
    bl = device_baseline(amx, ctxs, "two_fits")
    bl.fit(paths, perms=perms)
    host = Host(layers, torch.float32)
    bl.sync_to(host)
    ctx = ctxs[226]
    obs = torch.from_numpy(np.concatenate([p["observations"] for p in paths])).to(DEV)
    lens = np.array([len(p["returns"]) for p in paths])
    end = np.zeros(n, dtype=np.uint8)
    end[np.cumsum(lens) - 1] = 1
    grid = dict(lengths=torch.from_numpy(lens.astype(np.int32)).to(DEV),
                base=torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).to(DEV))
    v_dev = bl.predict_grid(n, int(lens.max()), len(lens), obs, ctx.S, torch.from_numpy(end).to(DEV), 1, **grid)
    v_dev = v_dev[:n].cpu().numpy()
    gap = float(np.max(np.abs(host.predict(feat) - v_dev)))
    print(f"host-after-sync_to vs predict_grid: {gap:.3g}")
    assert gap <= 2e-5 * max(1.0, float(np.max(np.abs(v_dev))))
    sd = host.optimizer.state_dict()
    assert len(sd["state"]) == 6 and all(int(s["step"]) == steps for s in sd["state"].values())
    check_state(bl, h32, h64, steps)

    # one more fit: on the device, on the synced host, on a device baseline built from the fp32
    # restatement's state (from_mjrl), and on the two restatements
    paths2 = make_paths(77, lens, 226)
    feat2, y2 = R.mlp_baseline_features(paths2), returns_of(paths2)
    perm2 = [np.random.RandomState(78).permutation(n)]
    bl2 = amx.DeviceMLPBaseline.from_mjrl(ctx, h32)
    assert (bl2.learn_rate, bl2.reg_coef, bl2.batch_size, bl2.epochs) == (LR, REG, 64, 1)
    assert bl2.betas == (0.9, 0.999) and bl2.eps == 1e-8 and bl2.adam_state()[0] == steps
    r32, r64 = h32.fit(feat2, y2, perm2), h64.fit(feat2, y2, perm2)
    out = bl.fit(paths2, return_errors=True, return_all_errors=True, perms=perm2)
    out2 = bl2.fit(paths2, return_errors=True, return_all_errors=True, perms=perm2)
    host.fit(feat2, y2, perm2)
    torch.cuda.synchronize()
    for o, b in ((out, bl), (out2, bl2)):
        check_returns(o, r32, r64)
        check_state(b, h32, h64, 2 * steps)
    check_state(bl, host, h64, 2 * steps)  # the host continued from sync_to, against the same yardstick


def test_refusals(amx, ctxs):
    """Unsupported shapes raise NotImplementedError and too few rows ValueError, before any
    launch: no optimizer state or workspace is created and no weight moves.  Prediction keeps
    accepting what the fit refuses."""
    ctx = ctxs[226]
    paths = make_paths(3, (128,), 226)
    cases = [(dict(batch_size=32), (128, 128)), ({}, (128, 128, 128)), ({}, (256, 128))]
    for kw, hidden in cases:
        layers = R.init_mlp_baseline(226, hidden, seed=1)
        bl = amx.DeviceMLPBaseline(ctx, layers, **kw)
        w0 = bl.W[0].clone()
        with pytest.raises(NotImplementedError):
            bl.fit(paths)
        assert bl._adam is None and bl._fit_work is None and torch.equal(bl.W[0], w0)
    obs = torch.from_numpy(paths[0]["observations"]).to(DEV)  # `bl` is the width-256 baseline
    end = torch.zeros(128, dtype=torch.uint8, device=DEV)
    end[-1] = 1
    v = bl.predict_grid(128, 128, 1, obs, 226, end, 1)[:128].cpu().numpy()
    np.testing.assert_allclose(v, R.mlp_baseline_predict(layers, R.mlp_baseline_features(paths)), rtol=2e-5, atol=1e-6)
    bl = amx.DeviceMLPBaseline(ctx, R.init_mlp_baseline(226, (128, 128), seed=1))
    with pytest.raises(ValueError):
        bl.fit(make_paths(3, (60, 40), 226))
    assert bl._adam is None and bl._fit_work is None
