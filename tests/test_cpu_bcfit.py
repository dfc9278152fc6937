"""CPU-only checks of the behaviour-cloning warm start: plan_bc_batches draws what the
reference's loop draws and leaves numpy's generator where the reference leaves it; the
workspace size (amx_bcfit_work) is pure host arithmetic; amx_bcfit_steps / amx_bcfit_eval
refuse bad arguments with AMX_E_INVAL and a message naming the entry point and the argument
before anything touches a GPU; and the fp32 restatement tests/bcfit_ref.py reproduces G17's
recorded reference run."""
import ctypes

import numpy as np
import pytest
import torch

import bcfit_ref as B
from amp_extensions_amd import _build, _native


@pytest.fixture(scope="module")
def lib():
    path = _build.build(verbose=False)
    return _native.load(path)


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_batch_plan_is_the_reference_draw():
    from amp_extensions_amd.bc import plan_bc_batches
    np.random.seed(77)
    direct = np.stack([np.random.choice(323, size=64) for _ in range(10)])
    after = np.random.get_state()
    np.random.seed(77)
    plan = plan_bc_batches(323, 2)
    assert plan.dtype == np.int32 and plan.shape == (2, 5, 64)
    assert np.array_equal(plan.reshape(10, 64), direct)
    assert same_state(np.random.get_state(), after)
    # 63 rows: int(63 / 64) = 0 steps, nothing drawn
    empty = plan_bc_batches(63, 3)
    assert empty.shape == (3, 0, 64) and same_state(np.random.get_state(), after)


def test_workspace_size_is_host_arithmetic(lib):
    # amx_bcfit_eval: one fp64 partial per workgroup, 1024 workgroups at most; amx_bcfit_steps: none
    assert lib.amx_bcfit_work(197, 36) == 1024 * 8
    assert lib.amx_bcfit_work(226, 28) == 1024 * 8
    assert lib.amx_bcfit_work(256, 64) == 1024 * 8
    for bad in ((197, 65), (257, 36), (0, 36), (197, 0)):
        assert lib.amx_bcfit_work(*bad) == -1
        assert b"amx_bcfit_work" in lib.amx_last_error()


def fake_ctx(S=197, A=36):
    """A zeroed amx_ctx stand-in with S and A set (device, n_cus, S, A lead the struct): every
    call below is refused before anything else of it is read."""
    buf = (ctypes.c_int * 512)()
    buf[2], buf[3] = S, A
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def steps(lib, ctx, n_steps=1, idx=4096, loss_type=0, N=64):
    d = ctypes.c_void_p(4096)  # non-null dummies: the argument checks never dereference them
    return lib.amx_bcfit_steps(ctx, N, d, 197, d, 36, ctypes.c_void_p(idx) if idx else None, n_steps, d, d, d, d,
                               1e-3, 0.9, 0.999, 1e-8, 0.0, loss_type, d, None)


def evaluate(lib, ctx, loss_type=0, N=64):
    d = ctypes.c_void_p(4096)
    return lib.amx_bcfit_eval(ctx, N, d, 197, d, 36, d, loss_type, d, d, None)


def test_argument_checks_come_before_the_gpu(lib):
    keep, ctx = fake_ctx()
    assert steps(lib, None) == -1
    assert b"amx_bcfit_steps" in lib.amx_last_error() and b"null ctx" in lib.amx_last_error()
    assert evaluate(lib, None) == -1
    assert b"amx_bcfit_eval" in lib.amx_last_error() and b"null ctx" in lib.amx_last_error()
    assert steps(lib, ctx, n_steps=-1) == -1
    assert b"amx_bcfit_steps" in lib.amx_last_error() and b"n_steps=-1" in lib.amx_last_error()
    assert steps(lib, ctx, idx=0) == -1
    assert b"amx_bcfit_steps" in lib.amx_last_error() and b"idx" in lib.amx_last_error()
    assert steps(lib, ctx, loss_type=2) == -1
    assert b"amx_bcfit_steps" in lib.amx_last_error() and b"loss_type=2" in lib.amx_last_error()
    assert evaluate(lib, ctx, loss_type=2) == -1
    assert b"amx_bcfit_eval" in lib.amx_last_error() and b"loss_type=2" in lib.amx_last_error()
    assert steps(lib, ctx, N=0) == -1 and b"N=0" in lib.amx_last_error()
    _, wide = fake_ctx(A=65)
    assert evaluate(lib, wide) == -1
    assert b"amx_bcfit_eval" in lib.amx_last_error() and b"A=65" in lib.amx_last_error()
    del keep


def test_python_refusals_need_no_gpu():
    """BC's refusals are decided from host-side fields alone."""
    from amp_extensions_amd.bc import BC

    class FC:
        def __init__(self, hidden):
            sizes = (197,) + hidden + (36,)
            self.fc_layers = [torch.nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]
            self.transformations = dict(in_shift=None, in_scale=None, out_shift=None, out_scale=None)

    class Policy:
        def __init__(self, hidden=(32, 32)):
            self.model = FC(hidden)
            self.log_std = torch.zeros(36, requires_grad=True)
            self.trainable_params = [p for l in self.model.fc_layers for p in l.parameters()] + [self.log_std]

    for exc, hidden, kw in ((NotImplementedError, (32, 32), dict(set_transforms=True)),
                            (NotImplementedError, (64, 64), {}),
                            (NotImplementedError, (32, 32), dict(batch_size=32)),
                            (ValueError, (32, 32), dict(loss_type="RWR"))):
        with pytest.raises(exc):
            BC([], Policy(hidden), **kw)
    pol = Policy()
    for opt in (torch.optim.SGD(pol.trainable_params, lr=1e-3), torch.optim.Adam(pol.trainable_params, amsgrad=True)):
        with pytest.raises(NotImplementedError):
            BC([], pol, optimizer=opt)
    bc = BC([], pol, lr=3e-4)
    assert type(bc.optimizer) is torch.optim.Adam and bc.optimizer.param_groups[0]["lr"] == 3e-4
    assert bc.device_bc is None and bc.logger.log == {}


@pytest.mark.parametrize("loss_type", ["MSE", "MLE"])
def test_fp32_restatement_reproduces_g17(golden, loss_type):
    """tests/bcfit_ref.py in fp32 against the reference's recorded run (two train() calls on one
    BC object): the final parameters and optimizer state within the device tests' tolerances."""
    from amp_extensions_amd.bc import plan_bc_batches
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    g, k = golden("g17_bc_fit.npz"), loss_type.lower()
    S, A = 197, 36
    obs, act = B.concat(B.make_paths([int(l) for l in g["lens"]], S, A, seed=int(g["path_seed"])))
    flat = pack_policy(*init_mlp_policy_params(S, A, seed=int(g["model_seed"]), init_log_std=-0.25))
    h = B.Host(flat, S, A, torch.float32, loss_type)
    np.random.seed(int(g["numpy_seed"]))
    res = [h.fit(obs, act, plan_bc_batches(len(obs), 2)) for _ in range(2)]
    ref = g[f"{k}_params"]
    assert np.max(np.abs(h.flat() - ref)) <= 2e-5 * max(1.0, float(np.max(np.abs(ref))))
    step, m, v = h.adam()
    assert step == int(g[f"{k}_step"]) == 20 and len(m) == int(g[f"{k}_n_state"])
    for i in range(len(m)):
        for mine, name in ((m[i], f"{k}_exp_avg_{i}"), (v[i], f"{k}_exp_avg_sq_{i}")):
            assert np.max(np.abs(mine - g[name])) <= 1e-4 * float(np.max(np.abs(g[name])))
    for c in range(2):
        assert abs(res[c][0] - g[f"{k}_loss_before"][c]) <= 1e-4 * abs(g[f"{k}_loss_before"][c])
        assert abs(res[c][2] - g[f"{k}_loss_after"][c]) <= 1e-4 * abs(g[f"{k}_loss_after"][c])
