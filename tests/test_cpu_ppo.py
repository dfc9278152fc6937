"""CPU-only checks of the PPO update: the fp32 restatement tests/ppo_ref.py reproduces G20's
recorded reference run bit for bit (first call against a snapshot, second call with the old mean
network tracking the new one) and does not when the second call keeps the snapshot form;
amx_ppo_steps / amx_ppo_old_ll refuse bad arguments with AMX_E_INVAL and a message naming the
entry point and the argument before anything touches a GPU; PPO's refusals need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_ref as R
from amp_extensions_amd import _build, _native

S, A = 197, 36
VARIANTS = ("default", "clipped")


@pytest.fixture(scope="module")
def lib():
    path = _build.build(verbose=False)
    return _native.load(path)


def g20_run(g, k, second):
    """The fp32 restatement over G20's two calls; the second in the form `second`."""
    from amp_extensions_amd.bc import plan_bc_batches
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    flat = pack_policy(*init_mlp_policy_params(S, A, seed=int(g["model_seed"]), init_log_std=-0.25))
    obs, act, adv = R.concat(R.make_paths([int(l) for l in g["lens"]], S, A, flat, seed=int(g["path_seed"])))
    h = R.Host(flat, S, A, torch.float32, lr=float(g[f"{k}_learn_rate"]), min_log_std=float(g[f"{k}_min_log_std"]))
    np.random.seed(int(g[f"{k}_numpy_seed"]))
    outs, flats = [], []
    for old in ("snapshot", second):
        outs.append(h.update(obs, act, adv, plan_bc_batches(len(obs), 2), old=old))
        flats.append(h.flat())
    return h, outs, flats


@pytest.mark.parametrize("k", VARIANTS)
def test_fp32_restatement_is_g20_bit_for_bit(golden, k):
    g = golden("g20_ppo_update.npz")
    h, outs, flats = g20_run(g, k, "tracks_mean")
    for call in range(2):
        assert np.array_equal(flats[call], g[f"{k}_params_{call}"]), f"call {call}"
        assert np.float32(outs[call]["kl_dist"]) == g[f"{k}_kl_dist"][call]
        assert np.float32(outs[call]["surr_after"] - outs[call]["surr_before"]) == g[f"{k}_surr_improvement"][call]
    step, m, v = h.adam()
    assert step == int(g[f"{k}_step"]) == 20 and len(m) == 7
    for i in range(7):
        assert np.array_equal(m[i], g[f"{k}_exp_avg_{i}"]) and np.array_equal(v[i], g[f"{k}_exp_avg_sq_{i}"])
    # the figures the GPU tests rely on
    assert [o["clamped"] for o in outs] == {"default": [9, 14], "clipped": [7, 14]}[k]
    assert [int(o["step_clipped"].sum()) for o in outs] == {"default": [5, 0], "clipped": [227, 6]}[k]


@pytest.mark.parametrize("k", VARIANTS)
def test_second_call_as_snapshot_is_not_the_reference(golden, k):
    g = golden("g20_ppo_update.npz")
    _, _, flats = g20_run(g, k, "snapshot")
    assert np.array_equal(flats[0], g[f"{k}_params_0"])
    assert not np.array_equal(flats[1], g[f"{k}_params_1"])


def fake_ctx(S=197, A=36):
    """A zeroed amx_ctx stand-in with S and A set (device, n_cus, S, A lead the struct): every
    call below is refused before anything else of it is read."""
    buf = (ctypes.c_int * 512)()
    buf[2], buf[3] = S, A
    return buf, ctypes.cast(buf, ctypes.c_void_p)


D = ctypes.c_void_p(4096)  # a non-null dummy: the argument checks never dereference it


def steps(lib, ctx, N=64, ldo=197, adv=D, ll_old=D, ls_old=D, mode=0, idx=D, n_steps=1, lr=3e-4, clip=0.2,
          clipped=D):
    return lib.amx_ppo_steps(ctx, N, D, ldo, D, 36, adv, ll_old, ls_old, mode, idx, n_steps, D, D, D, D, lr, 0.9,
                             0.999, 1e-8, clip, D, clipped, None)


def old_ll(lib, ctx, N=64, out=D):
    return lib.amx_ppo_old_ll(ctx, N, D, 197, D, 36, D, out, None)


def test_argument_checks_come_before_the_gpu(lib):
    keep, ctx = fake_ctx()

    def refused(rc, entry, word):
        err = lib.amx_last_error()
        assert rc == -1 and entry in err and word in err, err

    refused(steps(lib, None), b"amx_ppo_steps", b"null ctx")
    refused(old_ll(lib, None), b"amx_ppo_old_ll", b"null ctx")
    refused(steps(lib, ctx, n_steps=-1), b"amx_ppo_steps", b"n_steps=-1")
    refused(steps(lib, ctx, idx=None), b"amx_ppo_steps", b"idx")
    refused(steps(lib, ctx, N=0), b"amx_ppo_steps", b"N=0")
    refused(steps(lib, ctx, ldo=100), b"amx_ppo_steps", b"ldo=100")
    refused(steps(lib, ctx, adv=None), b"amx_ppo_steps", b"adv")
    refused(steps(lib, ctx, mode=2), b"amx_ppo_steps", b"old_mode=2")
    refused(steps(lib, ctx, mode=0, ll_old=None), b"amx_ppo_steps", b"ll_old")
    refused(steps(lib, ctx, mode=1, ls_old=None), b"amx_ppo_steps", b"log_std_old")
    refused(steps(lib, ctx, clipped=None), b"amx_ppo_steps", b"step_clipped")
    refused(steps(lib, ctx, lr=0.0), b"amx_ppo_steps", b"lr=0")
    refused(steps(lib, ctx, clip=1.5), b"amx_ppo_steps", b"clip_coef=1.5")
    refused(old_ll(lib, ctx, N=0), b"amx_ppo_old_ll", b"N=0")
    refused(old_ll(lib, ctx, out=None), b"amx_ppo_old_ll", b"ll_old")
    _, wide = fake_ctx(A=65)
    refused(steps(lib, wide), b"amx_ppo_steps", b"A=65")
    refused(old_ll(lib, wide), b"amx_ppo_old_ll", b"A=65")
    _, tall = fake_ctx(S=257)
    refused(steps(lib, tall, ldo=257), b"amx_ppo_steps", b"S=257")
    # the modes' unused pointer may be null; n_steps = 0 launches nothing
    assert steps(lib, ctx, mode=0, ls_old=None, n_steps=0) == 0
    assert steps(lib, ctx, mode=1, ll_old=None, n_steps=0) == 0
    del keep


def test_python_refusals_need_no_gpu():
    """PPO's refusals are decided from host-side fields alone."""
    from amp_extensions_amd.ppo import PPO

    class FC:
        def __init__(self, hidden):
            sizes = (197,) + hidden + (36,)
            self.fc_layers = [torch.nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]
            self.transformations = dict(in_shift=None, in_scale=None, out_shift=None, out_scale=None)

        def parameters(self):
            return [p for l in self.fc_layers for p in l.parameters()]

    class Policy:
        def __init__(self, hidden=(32, 32)):
            self.model, self.old_model = FC(hidden), FC(hidden)
            self.log_std = torch.zeros(36, requires_grad=True)
            self.trainable_params = self.model.parameters() + [self.log_std]

    with pytest.raises(NotImplementedError):
        PPO(None, Policy((64, 64)), None)
    with pytest.raises(NotImplementedError):
        PPO(None, Policy(), None, mb_size=32)
    pol = Policy()
    pol.model.transformations["in_shift"] = np.zeros(197)
    with pytest.raises(NotImplementedError):
        PPO(None, pol, None)

    pol = Policy()
    ppo = PPO("env", pol, "baseline", learn_rate=1e-3, seed=7)
    assert type(ppo.optimizer) is torch.optim.Adam and ppo.optimizer.param_groups[0]["lr"] == 1e-3
    assert (ppo.env, ppo.baseline, ppo.seed, ppo.running_score, ppo.device_ppo) == ("env", "baseline", 7, None, None)
    assert ppo.logger.log == {}
    for opt in (torch.optim.SGD(pol.trainable_params, lr=1e-3), torch.optim.Adam(pol.trainable_params, amsgrad=True)):
        ppo.optimizer = opt
        with pytest.raises(NotImplementedError):
            ppo.train_from_paths([])
        assert ppo.device_ppo is None and not opt.state
    # old_model sharing some of model's tensors and not others
    ppo.optimizer = torch.optim.Adam(pol.trainable_params)
    pol.old_model.fc_layers[0].weight.data = pol.model.fc_layers[0].weight.data
    with pytest.raises(NotImplementedError):
        ppo.train_from_paths([])
    assert ppo.device_ppo is None
