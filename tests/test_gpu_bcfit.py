"""GPU parity of the device behaviour-cloning warm start (amx_bcfit_steps / amx_bcfit_eval;
DeviceBC, BC) against the reference's BC.train (mjrl/mjrl/algos/behavior_cloning.py:14-145).

The comparator is tests/bcfit_ref.py: the reference loop restated in torch on the CPU, run in
fp64 (the yardstick) and in fp32 (the reference's own arithmetic).  Every comparison first
asserts that fp32 alone is within a quarter of the tolerance of fp64 (so the inputs do not sit
on one of Adam's lr * g / (|g| + eps) cliffs), then that the device is within the tolerance of
fp64 (test_gpu_vfit.py's `check`).

Tolerances (DESIGN.md's table, as the value fit's): 2e-5 * max(1, max|ref|) for theta, 1e-4
relative for loss_before / loss_after / the epoch totals and 1e-4 * max|ref| per tensor for
exp_avg / exp_avg_sq.  G17 (tests/golden/make_golden_bc.py) is the reference's own run of two
consecutive train() calls; there the recorded fp32 results take the place of the fp32
restatement.
"""
import functools

import numpy as np
import pytest
import torch

import bcfit_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["W1", "b1", "W2", "b2", "W3", "b3", "log_std"]

TOL_W = lambda ref: 2e-5 * max(1.0, float(np.max(np.abs(ref))))  # noqa: E731  theta, means
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


def check_theta(theta, flat32, flat64, S, A):
    for n, d, a, b in zip(NAMES, B.split_flat(theta, S, A), B.split_flat(flat32, S, A), B.split_flat(flat64, S, A)):
        check(n, d, a, b, TOL_W)


def check_adam(state, adam32, adam64, steps):
    """state / adam32 / adam64: (step, [exp_avg], [exp_avg_sq]) over the same parameters."""
    assert state[0] == adam32[0] == adam64[0] == steps
    assert len(state[1]) == len(adam32[1]) == len(adam64[1])
    for which, k in (("exp_avg", 1), ("exp_avg_sq", 2)):
        for n, d, a, b in zip(NAMES, state[k], adam32[k], adam64[k]):
            check(f"{which} {n}", np.asarray(d).reshape(b.shape), a, b, TOL_M)


def check_losses(out, r32, r64):
    check("loss_before", out[0], r32[0], r64[0], TOL_S)
    check("epoch totals", out[1], r32[1], r64[1], TOL_S)
    check("loss_after", out[2], r32[2], r64[2], TOL_S)


# ---- cases (host part cached: computed once per module) ---------------------------------------

CASES = {
    #  name        S    A   lens                epochs
    "one_step": (197, 36, (64,), 1),
    "ragged": (197, 36, (70, 130, 3, 120), 2),
    # N = 128 as two paths: with lens (128,) these seeds put the fp32 restatement itself on an Adam
    # cliff in step 2 (its exp_avg is 9.6 x tol/4 from fp64; `check` refuses such inputs); with
    # (100, 28) the fp32-vs-fp64 gaps are 0.02 x tol/4 on the moments and 0.05 x on theta
    "other": (226, 28, (100, 28), 1),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(flat theta, obs, act, batches) of a case: the issue's seeds."""
    from amp_extensions_amd.bc import plan_bc_batches
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    S, A, lens, epochs = CASES[name]
    obs, act = B.concat(B.make_paths(lens, S, A, seed=5))
    flat = pack_policy(*init_mlp_policy_params(S, A, seed=123, init_log_std=-0.25))
    np.random.seed(77)
    return flat, obs, act, plan_bc_batches(len(obs), epochs)


@functools.lru_cache(maxsize=None)
def reference(name, loss_type):
    """(fp32 host, fp64 host, fp32 results, fp64 results) of a case after one fit."""
    S, A, _, _ = CASES[name]
    flat, obs, act, batches = inputs(name)
    h32, h64 = B.Host(flat, S, A, torch.float32, loss_type), B.Host(flat, S, A, torch.float64, loss_type)
    return h32, h64, h32.fit(obs, act, batches), h64.fit(obs, act, batches)


@pytest.fixture(scope="module")
def amx():
    import amp_extensions_amd as amx
    return amx


@pytest.fixture(scope="module")
def ctxs(amx):
    return {S: amx.AmxContext(S, A, n_models=1, hidden=16, n_hidden=1, feat_dim=256, device=DEV)
            for S, A in ((197, 36), (226, 28))}


def device_fit(amx, ctxs, name, loss_type, **kw):
    S, _, _, epochs = CASES[name]
    flat, obs, act, batches = inputs(name)
    dbc = amx.DeviceBC(ctxs[S], flat, loss_type=loss_type)
    out = dbc.fit(obs, act, epochs, batches=batches, **kw)
    torch.cuda.synchronize()
    return dbc, out


def trained(state, n):
    return state[0], state[1][:n], state[2][:n]


def run_case(amx, ctxs, name, loss_type):
    S, A, _, _ = CASES[name]
    h32, h64, r32, r64 = reference(name, loss_type)
    dbc, out = device_fit(amx, ctxs, name, loss_type)
    check_losses(out, r32, r64)
    check("step losses", dbc.step_losses, r32[3], r64[3], TOL_S)
    check_theta(dbc.theta.cpu().numpy(), h32.flat(), h64.flat(), S, A)
    n = 7 if loss_type == "MLE" else 6
    assert len(h64.adam()[1]) == n
    check_adam(trained(dbc.adam_state(), n), h32.adam(), h64.adam(), h64.adam()[0])
    return dbc


# ---- tests -----------------------------------------------------------------------------------

@pytest.mark.parametrize("loss_type", ["MSE", "MLE"])
def test_one_step(amx, ctxs, loss_type):
    """N = 64: one step from a fresh state.  The 2 / (64 A) (MSE) or 1 / (64 sigma^2) (MLE)
    factor, tanh' and the bias correction at t = 1 all show in theta (every weight moves by
    about lr) and in exp_avg = 0.1 g.  Under MSE log_std has no gradient: not a bit of it moves
    and it gets no moment; under MLE it moves and has one."""
    dbc = run_case(amx, ctxs, "one_step", loss_type)
    A = 36
    step, m, v = dbc.adam_state()
    assert step == 1
    ls0, ls1 = inputs("one_step")[0][-A:], dbc.theta[-A:].cpu().numpy()
    if loss_type == "MSE":
        assert np.array_equal(ls0, ls1)
        assert not m[6].any() and not v[6].any()
    else:
        assert np.all(np.abs(ls1 - ls0) > 5e-4)
        assert m[6].abs().min() > 0 and v[6].min() > 0


@pytest.mark.parametrize("loss_type", ["MSE", "MLE"])
def test_ragged_gather_with_replacement(amx, ctxs, loss_type):
    """N = 323 (paths of 70, 130, 3, 120 rows), 2 epochs x 5 steps: batches drawn with
    replacement gather repeated rows and rows of several paths."""
    batches = inputs("ragged")[3]
    assert batches.shape == (2, 5, 64)
    assert any(len(set(b)) < 64 and len({int(np.searchsorted([70, 200, 203], i, side="right")) for i in b}) >= 3
               for b in batches.reshape(-1, 64).tolist())
    dbc = run_case(amx, ctxs, "ragged", loss_type)
    assert dbc.adam_state()[0] == 10


def test_other_size(amx, ctxs):
    """S / A = 226 / 28 (S no multiple of 32, A no multiple of 16), N = 128: two steps.  theta
    and the moments hold exactly amx_npg_param_count floats: the kernel's padding exists only
    in its LDS image and is never written back."""
    dbc = run_case(amx, ctxs, "other", "MSE")
    P = int(ctxs[226].lib.amx_npg_param_count(226, 28))
    assert P == 32 * 226 + 32 + 32 * 32 + 32 + 28 * 32 + 28 + 28
    assert dbc.theta.numel() == P and all(t.numel() == P for t in dbc._adam[:2])
    assert dbc.adam_state()[0] == 2


class _FC(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.fc_layers = torch.nn.ModuleList(layers)
        self.transformations = dict(in_shift=None, in_scale=None, out_shift=None, out_scale=None)


class _MjrlMLP:
    """The attribute layout of mjrl's MLP policy (gaussian_mlp.py:7-92): model / old_model with
    fc_layers, log_std / old_log_std, trainable_params / old_params, get_param_values and
    set_param_values(new_params, set_new, set_old) with the log_std clamp."""

    def __init__(self, S, A, hidden=(32, 32), seed=123, init_log_std=-0.25, min_log_std=-3.0):
        from amp_extensions_amd.policy import init_mlp_policy_params
        self.n, self.m, self.min_log_std = S, A, min_log_std
        pw, log_std = init_mlp_policy_params(S, A, hidden, seed=seed, init_log_std=init_log_std)

        def fc():
            layers = []
            for W, b in pw:
                lin = torch.nn.Linear(W.shape[1], W.shape[0])
                lin.weight.data, lin.bias.data = W.clone().float(), b.clone().float()
                layers.append(lin)
            return _FC(layers)
        self.model, self.old_model = fc(), fc()
        self.log_std = torch.autograd.Variable(log_std.clone().float(), requires_grad=True)
        self.old_log_std = torch.autograd.Variable(log_std.clone().float())
        self.trainable_params = list(self.model.parameters()) + [self.log_std]
        self.old_params = list(self.old_model.parameters()) + [self.old_log_std]
        self.log_std_val = np.float64(self.log_std.data.numpy().ravel())
        self.param_shapes = [p.data.numpy().shape for p in self.trainable_params]
        self.param_sizes = [p.data.numpy().size for p in self.trainable_params]

    def get_param_values(self):
        return np.concatenate([p.contiguous().view(-1).data.numpy() for p in self.trainable_params]).copy()

    def set_param_values(self, new_params, set_new=True, set_old=True):
        for on, params in ((set_new, self.trainable_params), (set_old, self.old_params)):
            if not on:
                continue
            i = 0
            for p, shape, n in zip(params, self.param_shapes, self.param_sizes):
                p.data = torch.from_numpy(new_params[i:i + n].reshape(shape)).float()
                i += n
            params[-1].data = torch.clamp(params[-1], self.min_log_std).data
        if set_new:
            self.log_std_val = np.float64(self.log_std.data.numpy().ravel())


def optimizer_state(opt, params):
    st = [opt.state[p] for p in params if p in opt.state]
    assert len({int(s["step"]) for s in st}) == 1
    return int(st[0]["step"]), [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st]


@pytest.mark.parametrize("loss_type", ["MSE", "MLE"])
def test_g17_two_reference_trains(amx, ctxs, golden, loss_type, capsys):
    """The reference's BC.train called twice on one BC object (2 epochs of 5 steps each; the
    second call resumes Adam at step 10 and keeps drawing from the same numpy stream)
    reproduces through the drop-in: final parameters, the optimizer's state (six entries under
    MSE, seven under MLE) and the logger's loss_before / loss_after of each call."""
    g, k = golden("g17_bc_fit.npz"), loss_type.lower()
    S, A, lens = 197, 36, [int(l) for l in g["lens"]]
    paths = B.make_paths(lens, S, A, seed=int(g["path_seed"]))
    obs, act = B.concat(paths)
    pol = _MjrlMLP(S, A, seed=int(g["model_seed"]), min_log_std=-2.0)
    flat0 = pol.get_param_values()

    np.random.seed(int(g["numpy_seed"]))
    h64 = B.Host(flat0, S, A, torch.float64, loss_type)
    r64 = [h64.fit(obs, act, amx.plan_bc_batches(len(obs), 2)) for _ in range(2)]

    bc = amx.BC(paths, policy=pol, epochs=2, batch_size=64, lr=1e-3, loss_type=loss_type, ctx=ctxs[S])
    np.random.seed(int(g["numpy_seed"]))
    bc.train(suppress_fit_tqdm=True)
    bc.train(suppress_fit_tqdm=True)
    torch.cuda.synchronize()
    printed = capsys.readouterr().out
    assert printed.count("Num samples: 323") == 2 and printed.count("Total loss for epoch") == 4

    n = int(g[f"{k}_n_state"])
    assert n == (7 if loss_type == "MLE" else 6) and len(bc.optimizer.state) == n
    check_theta(pol.get_param_values(), g[f"{k}_params"], h64.flat(), S, A)
    ref32 = (int(g[f"{k}_step"]), [g[f"{k}_exp_avg_{i}"] for i in range(n)], [g[f"{k}_exp_avg_sq_{i}"] for i in range(n)])
    check_adam(optimizer_state(bc.optimizer, pol.trainable_params), ref32, h64.adam(), 20)
    assert bc.logger.log["epoch"] == [2, 2] and len(bc.logger.log["time"]) == 2
    for c in range(2):
        check(f"loss_before {c}", bc.logger.log["loss_before"][c], g[f"{k}_loss_before"][c], r64[c][0], TOL_S)
        check(f"loss_after {c}", bc.logger.log["loss_after"][c], g[f"{k}_loss_after"][c], r64[c][2], TOL_S)


def test_write_back_clamps_the_policy_not_theta(amx, ctxs):
    """MLE with min_log_std = -0.2, above every trained value (about -0.24): the policy gets
    the reference's write-back (log_std, old_log_std and log_std_val clamped, old_model = model)
    while DeviceBC.theta keeps the unclamped values; a DevicePolicy built from the policy
    computes the trained means."""
    S, A, _, epochs = CASES["ragged"]
    _, obs, act, _ = inputs("ragged")
    h32, h64, _, _ = reference("ragged", "MLE")
    paths = B.make_paths(CASES["ragged"][2], S, A, seed=5)
    pol = _MjrlMLP(S, A, seed=123, min_log_std=-0.2)
    assert np.array_equal(pol.get_param_values(), inputs("ragged")[0])
    bc = amx.BC(paths, policy=pol, epochs=epochs, loss_type="MLE", ctx=ctxs[S])
    np.random.seed(77)
    bc.train(suppress_fit_tqdm=True)
    torch.cuda.synchronize()
    theta = bc.device_bc.theta.cpu().numpy()
    check_theta(theta, h32.flat(), h64.flat(), S, A)
    assert theta[-A:].max() < -0.2
    clamp = np.full(A, np.float32(-0.2))
    assert np.array_equal(pol.log_std.data.numpy(), clamp) and np.array_equal(pol.old_log_std.data.numpy(), clamp)
    assert np.array_equal(pol.log_std_val, np.float64(clamp))
    for p, q in zip(pol.trainable_params, pol.old_params):
        assert torch.equal(p.data, q.data)
    assert np.array_equal(pol.get_param_values()[:-A], theta[:-A])

    dp = amx.DevicePolicy.from_mjrl(ctxs[S], pol)
    ob = obs[:128]
    out = torch.empty(128, A, dtype=torch.float64, device=DEV)
    mean = torch.empty(128, A, dtype=torch.float32, device=DEV)
    dp.act(torch.from_numpy(ob).to(DEV), 128, out, counter=0, eval_mode=True, mean_out=mean)
    with torch.no_grad():
        m32, m64 = (h.mean(h.data(ob, act[:128])[0]).numpy() for h in (h32, h64))
    check("means after the warm start", mean.cpu().numpy(), m32, m64, TOL_W)
    assert np.array_equal(out.cpu().numpy(), mean.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("loss_type", ["MSE", "MLE"])
def test_launch_cut_changes_no_bit(amx, ctxs, loss_type):
    """The ragged fit in launches of at most 3 steps (10 steps: 3 + 3 + 3 + 1) against one launch."""
    a, out_a = device_fit(amx, ctxs, "ragged", loss_type)
    b, out_b = device_fit(amx, ctxs, "ragged", loss_type, max_steps_per_launch=3)
    assert torch.equal(a.theta, b.theta)
    assert all(torch.equal(x, y) for x, y in zip(a._adam, b._adam))
    assert np.array_equal(a.step_losses, b.step_losses) and len(a.step_losses) == 10
    assert out_a == out_b


def test_fit_is_deterministic(amx, ctxs):
    a, out_a = device_fit(amx, ctxs, "ragged", "MLE")
    b, out_b = device_fit(amx, ctxs, "ragged", "MLE")
    assert torch.equal(a.theta, b.theta)
    assert all(torch.equal(x, y) for x, y in zip(a._adam, b._adam))
    assert np.array_equal(a.step_losses, b.step_losses) and out_a == out_b


def test_resume_through_the_optimizer(amx, ctxs):
    """A fresh BC built on the same policy with the first object's optimizer continues to the
    same theta as one object training twice, bit for bit."""
    S, A, lens, epochs = CASES["ragged"]
    paths = B.make_paths(lens, S, A, seed=5)
    thetas = []
    for fresh in (False, True):
        pol = _MjrlMLP(S, A, seed=123)
        bc = amx.BC(paths, policy=pol, epochs=epochs, loss_type="MLE", ctx=ctxs[S])
        np.random.seed(77)
        bc.train(suppress_fit_tqdm=True)
        if fresh:
            bc = amx.BC(paths, policy=pol, epochs=epochs, loss_type="MLE", optimizer=bc.optimizer, ctx=ctxs[S])
        bc.train(suppress_fit_tqdm=True)
        assert optimizer_state(bc.optimizer, pol.trainable_params)[0] == 20
        thetas.append((pol.get_param_values(), bc.device_bc.theta.cpu().numpy()))
    assert np.array_equal(thetas[0][0], thetas[1][0]) and np.array_equal(thetas[0][1], thetas[1][1])


def test_refusals(amx, ctxs):
    """Unsupported configurations raise before anything is launched or allocated: no device
    object exists afterwards and the policy's parameters are untouched."""
    S, A = 197, 36
    paths = B.make_paths((64,), S, A, seed=5)

    def refused(exc, hidden=(32, 32), transform=False, opt=None, **kw):
        pol = _MjrlMLP(S, A, hidden=hidden, seed=123)
        if transform:
            pol.model.transformations["in_shift"] = np.zeros(S)
        before = pol.get_param_values()
        optimizer = opt(pol.trainable_params) if opt else None
        made = []
        with pytest.raises(exc):
            made.append(amx.BC(paths, policy=pol, optimizer=optimizer, ctx=ctxs[S], **kw))
        assert not made and np.array_equal(pol.get_param_values(), before)
        assert optimizer is None or not optimizer.state

    refused(NotImplementedError, set_transforms=True)
    refused(NotImplementedError, transform=True)
    refused(NotImplementedError, hidden=(64, 64))
    refused(NotImplementedError, batch_size=32)
    refused(NotImplementedError, opt=lambda p: torch.optim.SGD(p, lr=1e-3))
    refused(NotImplementedError, opt=lambda p: torch.optim.Adam(p, lr=1e-3, amsgrad=True))
    refused(ValueError, loss_type="RWR")
