"""GAILCost.update_disc / compute_chi2_distance and AgentReplayBuffer on the GPU (amx_dfit_step,
amx_gemm_nn_f32, amx_gemm_tn_f32).

Comparators: fixture G16 (tests/golden/make_golden_dfit.py: the reference's own update_disc, two
blocks of three steps) and, at shapes G16 does not hold, the closed-form restatement
tests/dfit_ref.py in fp64 (the yardstick) and fp32.

The metric is the update, not the weight (at lr 1e-5 a step moves a weight by ~1e-6 of its size):
max |dW_dev - dW_ref| / max |dW_ref| per tensor with dW = W_after - W_init; optimizer state is
compared directly, max |s - s_ref| / max |s_ref| per tensor.  Tolerances, measured by the generator
as the distance of the reference's fp32 run from the fp64 restatement:
    block     dW        state
    sgd_ls    4.27e-4   1.47e-7
    adam_ll   2.01e-5   5.86e-7
TOL_DW = 2e-3 and TOL_STATE = 3e-6 are 4 x the largest, rounded up to one significant digit: the
fp32 comparator within a quarter of the tolerance, the device (fp32 sums in another order)
within the tolerance.  Metrics and chi^2: 1e-4 relative (the project's tolerance for costs).
The products: |err| <= 2 K 2^-24 (|A| |B|) elementwise, the fp32 FMA-chain bound."""
import os

import numpy as np
import pytest
import torch

import dfit_ref as R

pytestmark = pytest.mark.gpu

G = R.G16
TOL_DW, TOL_STATE, TOL_METRIC = 2e-3, 3e-6, 1e-4
DEV = "cuda"


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g16_disc_update.npz"))


@pytest.fixture(scope="module")
def ctx():
    from amp_extensions_amd.engine import AmxContext
    return AmxContext(4, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=128, device=DEV)


# ---- the two products -----------------------------------------------------------------------

def _pad(x, rows, cols):
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def _up(x, m):
    return (x + m - 1) // m * m


def _bound(A, B, K):
    return 2.0 * K * 2.0 ** -24 * (A.double().abs() @ B.double().abs())


PRODUCT_CASES = [(rows, n, k, epi) for rows in (37, 70, 192) for n, k in ((64, 96), (96, 160), (160, 64))
                 for epi in (False, True)]


@pytest.mark.parametrize("rows,n,k,epi", PRODUCT_CASES)
def test_gemm_nn_f32(ctx, rows, n, k, epi):
    from amp_extensions_amd import _native as N
    rs = torch.Generator().manual_seed(rows * 1000 + n + k)
    Mp, Np, Kp = _up(rows, 64), _up(n, 128) if n > 64 else 64, _up(k, 128) if k > 64 else 64
    A = _pad(torch.randn(rows, k, generator=rs), Mp, Kp)
    B = _pad(torch.randn(k, n, generator=rs), Kp, Np)
    mask = torch.randn(64, Np, generator=rs) if epi else None   # rows wrap: r % 64
    want = A.double() @ B.double()
    if epi:
        want = want * (mask.repeat(Mp // 64, 1) > 0)
    Ad, Bd, Md = A.to(DEV), B.to(DEV), (mask.to(DEV) if epi else None)
    outs = []
    for _ in range(2):
        C = torch.full((Mp, Np), float("nan"), device=DEV)
        N.check(ctx.lib.amx_gemm_nn_f32(ctx.h, Mp, Np, Kp, Ad.data_ptr(), Kp, Bd.data_ptr(), Np, C.data_ptr(), Np,
                                        N.ptr(Md), Np, 64 if epi else 0, ctx.stream), "amx_gemm_nn_f32")
        outs.append(C.cpu())
    assert torch.equal(outs[0], outs[1])
    err = (outs[0].double() - want).abs()
    assert bool((err <= _bound(A, B, Kp)).all()), float(err.max())


@pytest.mark.parametrize("rows,n,k,epi", PRODUCT_CASES)
def test_gemm_tn_f32(ctx, rows, n, k, epi):
    """C = A^T B over R rows (all of them random, so the column sums' prefix `rows` matters)."""
    from amp_extensions_amd import _native as N
    rs = torch.Generator().manual_seed(rows * 1000 + n + k + 1)
    Rp, Np, Mp = _up(rows, 32), _up(n, 128) if n > 64 else 64, _up(k, 128) if k > 64 else 64
    A = torch.randn(Rp, Mp, generator=rs)
    A[:, k:] = 0
    B = torch.randn(Rp, Np, generator=rs)
    B[:, n:] = 0
    mask = torch.randn(Mp, Np, generator=rs) if epi else None
    want = A.double().T @ B.double()
    if epi:
        want = want * (mask > 0)
    want_cs = A[:rows].double().sum(0)
    Ad, Bd, Md = A.to(DEV), B.to(DEV), (mask.to(DEV) if epi else None)
    outs = []
    for _ in range(2):
        C = torch.full((Mp, Np), float("nan"), device=DEV)
        cs = torch.full((Mp,), float("nan"), device=DEV) if epi else None
        N.check(ctx.lib.amx_gemm_tn_f32(ctx.h, Rp, Mp, Np, Ad.data_ptr(), Mp, Bd.data_ptr(), Np, C.data_ptr(), Np,
                                        N.ptr(Md), Np, N.ptr(cs), rows, ctx.stream), "amx_gemm_tn_f32")
        outs.append((C.cpu(), cs.cpu() if epi else None))
    assert torch.equal(outs[0][0], outs[1][0])
    err = (outs[0][0].double() - want).abs()
    assert bool((err <= _bound(A.T, B, Rp)).all()), float(err.max())
    if epi:
        assert torch.equal(outs[0][1], outs[1][1])
        cerr = (outs[0][1].double() - want_cs).abs()
        assert bool((cerr <= 2.0 * rows * 2.0 ** -24 * A[:rows].double().abs().sum(0)).all()), float(cerr.max())


def test_gemm_refuses_bad_shapes(ctx):
    from amp_extensions_amd import _native as N
    x = torch.zeros(64, 64, device=DEV)
    p = x.data_ptr()
    assert ctx.lib.amx_gemm_nn_f32(ctx.h, 63, 64, 64, p, 64, p, 64, p, 64, None, 0, 0, ctx.stream) != 0
    assert ctx.lib.amx_gemm_nn_f32(ctx.h, 64, 64, 48, p, 64, p, 64, p, 64, None, 0, 0, ctx.stream) != 0
    assert ctx.lib.amx_gemm_tn_f32(ctx.h, 64, 64, 64, p, 64, p, 64, p, 64, None, 0, p, 65, ctx.stream) != 0
    torch.cuda.synchronize()


# ---- G16 on the device ----------------------------------------------------------------------

def _g16_cost(cfg, gemm="f16x3", device_adds=(1,)):
    """The replay ring filled by G16's three adds (the listed ones from device tensors) and the
    GAILCost of a block, built in the generator's order."""
    from amp_extensions_amd.costs import GAILCost
    from amp_extensions_amd.datasets import AgentReplayBuffer
    expert, adds, agent = R.g16_inputs()
    rb = AgentReplayBuffer(device=DEV, max_size=G["max_size"])
    for i, (s, s2) in enumerate(adds):
        rb.add(*((s.to(DEV), s2.to(DEV)) if i in device_adds else (s, s2)))
    gc = GAILCost(expert, agent_rb=rb, hidden_dims=list(G["hidden"]), seed=cfg["seed"], disc_loss_type=cfg["loss"],
                  disc_opt=cfg["opt"], disc_opt_args=dict(cfg["args"]), gemm=gemm, device=DEV)
    return gc, rb, expert, agent


class _Draws:
    """Record np.random.randint's results."""

    def __enter__(self):
        self.draws, self.real = [], np.random.randint

        def logged(*a, **k):
            v = self.real(*a, **k)
            self.draws.append(np.asarray(v).copy())
            return v
        np.random.randint = logged
        return self.draws

    def __exit__(self, *exc):
        np.random.randint = self.real


def _state_keys(opt):
    return [("buf", "momentum_buffer")] if opt == "sgd" else [("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")]


@pytest.mark.parametrize("name", list(G["blocks"]))
def test_g16_on_device(g16, name):
    cfg = G["blocks"][name]
    gc, rb, expert, agent = _g16_cost(cfg)
    init = R.init_weights(2 * G["S"], G["hidden"], cfg["seed"])
    assert len(rb) == G["max_size"] and torch.equal(torch.cat([rb.states, rb.next_states], -1).cpu(), agent)
    with _Draws() as draws:
        mets = [gc.update_disc(R.g16_mb(cfg, k)) for k in range(G["steps"])]
        n_steps = len(draws)
        chi2 = gc.compute_chi2_distance()
    per = n_steps // G["steps"]
    assert per == (1 if cfg["mb_seeds"] else 2) and len(draws) == n_steps + 1
    for k in range(G["steps"]):
        assert np.array_equal(draws[k * per + per - 1], g16[f"{name}_idx_e"][k])
        if per == 2:
            assert np.array_equal(draws[k * per], g16[f"{name}_idx_m"][k])
    assert np.array_equal(draws[-1], g16[f"{name}_chi2_idx"])
    for k in range(G["steps"]):
        for j, key in enumerate(R.METRICS):
            ref = g16[f"{name}_metrics"][k][j]
            print(f"{name} step {k} {key}: device {mets[k][key]!r} reference {ref!r}")
            assert isinstance(mets[k][key], float)
            assert abs(mets[k][key] - ref) <= TOL_METRIC * abs(ref), (k, key)
        if cfg["loss"] == "least_squares":
            for j, key in enumerate(("expert_acc", "mb_acc")):
                v = mets[k][key]
                assert torch.is_tensor(v) and v.dim() == 0 and v.dtype == torch.float32
                assert abs(float(v) - g16[f"{name}_acc"][k][j]) <= TOL_METRIC
        else:
            assert "expert_acc" not in mets[k]
    print(f"{name} chi2: device {chi2!r} reference {float(g16[f'{name}_chi2'])!r}")
    assert isinstance(chi2, float) and abs(chi2 - float(g16[f"{name}_chi2"])) <= TOL_METRIC * float(g16[f"{name}_chi2"])
    sd = gc.disc.state_dict()
    assert list(sd) == list(R.KEYS)
    opt = gc.disc_opt
    for j, (key, p) in enumerate(zip(R.KEYS, gc.disc.parameters())):
        assert sd[key].shape == init[j].shape
        e = R.update_error(sd[key], g16[f"{name}_p{j}"], init[j])
        print(f"{name} {R.NAMES[j]}: dW error {e:.3e} (tol {TOL_DW:.0e})")
        assert e <= TOL_DW, (R.NAMES[j], e)
        for fk, tk in _state_keys(cfg["opt"]):
            e = R.state_error(opt.state[p][tk], g16[f"{name}_p{j}_{fk}"])
            print(f"{name} {R.NAMES[j]} {tk}: error {e:.3e} (tol {TOL_STATE:.0e})")
            assert e <= TOL_STATE, (R.NAMES[j], tk, e)
        if cfg["opt"] != "sgd":
            assert float(opt.state[p]["step"]) == float(g16[f"{name}_step"])


# ---- against the fp64 restatement at the smallest ragged shape ------------------------------

S_SMALL, HID_SMALL, BS_SMALL = 24, [64, 32], 37


def _small(loss, opt, seed=100, lr=None, **kw):
    from amp_extensions_amd.costs import GAILCost
    args = {"lr": lr or 1e-5, "momentum": 0.9} if opt == "sgd" else {"lr": lr or 1e-3}
    expert = R.synthetic_rows(90, S_SMALL, 61, 0.5, 0.3)
    gc = GAILCost(expert, hidden_dims=list(HID_SMALL), seed=seed, disc_loss_type=loss, disc_opt=opt,
                  disc_opt_args=args, device=DEV, **kw)
    return gc, expert, args


def _dev_weights(gc):
    return [v.clone() for v in gc.disc.state_dict().values()]


def _dev_state(gc, key):
    opt = gc.disc_opt
    return [opt.state[p][key].clone() for p in gc.disc.parameters()]


@pytest.mark.parametrize("loss", ["least_squares", "log_likelihood"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_against_fp64_restatement(loss, opt):
    """D = 48, hidden [64, 32] (one tile per product), bs = 37: Bt - bs padded rows are live in
    every launch.  Both optimizers at lr 1e-3: at SGD's default 1e-5 the log-likelihood update is
    so small that the rounding of the fp32 weight itself (half an ulp of W) is 8e-4 of it on the
    CPU, fp32 against fp64, beyond the precondition of a quarter of TOL_DW; at 1e-3 the
    comparison is about the gradient (G16's sgd_ls block holds the default rate)."""
    gc, expert, args = _small(loss, opt, lr=1e-3)
    init = R.init_weights(2 * S_SMALL, HID_SMALL, 100)
    assert all(torch.equal(a, b) for a, b in zip(init, _dev_weights(gc)))
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 70 + k, 0.7, -0.2) for k in range(3)]
    with _Draws() as draws:
        mets = [gc.update_disc(mb) for mb in mbs]
    batches = [(expert[draws[k]], mbs[k]) for k in range(3)]
    p1 = args.get("momentum", 1e-8)
    r64, r32 = (R.restate(init, batches, loss, opt, args["lr"], p1, 0.5, 0.05, 10.0, dt)
                for dt in (torch.float64, torch.float32))
    for k in range(3):
        for key in R.METRICS:
            ref = r64["metrics"][k][key]
            assert abs(r32["metrics"][k][key] - ref) <= 0.25 * TOL_METRIC * abs(ref), (k, key)
            assert abs(mets[k][key] - ref) <= TOL_METRIC * abs(ref), (k, key, mets[k][key], ref)
    w = _dev_weights(gc)
    for j in range(6):
        e32, ed = (R.update_error(x[j], r64["weights"][j], init[j]) for x in (r32["weights"], w))
        print(f"{loss} {opt} {R.NAMES[j]}: dW fp32 {e32:.3e} device {ed:.3e}")
        assert e32 <= 0.25 * TOL_DW, (R.NAMES[j], e32)
        assert ed <= TOL_DW, (R.NAMES[j], ed)
    for tk, sk in ([("momentum_buffer", "s1")] if opt == "sgd" else [("exp_avg", "s1"), ("exp_avg_sq", "s2")]):
        st = _dev_state(gc, tk)
        for j in range(6):
            e32, ed = (R.state_error(x[j], r64["state"][sk][j]) for x in (r32["state"][sk], st))
            print(f"{loss} {opt} {R.NAMES[j]} {tk}: fp32 {e32:.3e} device {ed:.3e}")
            assert e32 <= 0.25 * TOL_STATE, (R.NAMES[j], tk, e32)
            assert ed <= TOL_STATE, (R.NAMES[j], tk, ed)


def test_chi2_samples_the_larger_buffer():
    """n >= Ne: all expert rows, Ne sampled buffer rows (the branch G16 does not take)."""
    from amp_extensions_amd.datasets import AgentReplayBuffer
    gc, expert, _ = _small("least_squares", "sgd")
    rows = R.synthetic_rows(130, S_SMALL, 77, 0.7, -0.2)
    rb = AgentReplayBuffer(device=DEV, max_size=100)
    rb.add(rows[:, :S_SMALL], rows[:, S_SMALL:])
    gc.online_rb = rb
    np.random.seed(5)
    got = gc.compute_chi2_distance()
    np.random.seed(5)
    idx = np.random.randint(0, 100, size=90)
    want = R.chi2(R.init_weights(2 * S_SMALL, HID_SMALL, 100), expert, rows[-100:][idx], 0.5, torch.float64)
    assert abs(got - want) <= TOL_METRIC * abs(want)


# ---- padding, determinism, degenerate rows --------------------------------------------------

def _run(gc, mbs, seed=3):
    np.random.seed(seed)
    return [gc.update_disc(mb) for mb in mbs]


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_padding_inert_and_deterministic(opt):
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 80 + k, 0.7, -0.2) for k in range(5)]
    runs = []
    for _ in range(2):
        gc, _, _ = _small("least_squares", opt)
        _run(gc, mbs)
        (W0, b0, _, _, _), (W1, b1, _, _, _) = gc.dev_layers
        t = gc._train
        runs.append([x.clone() for x in (W0, b0, W1, b1, gc.w3, t.b2, t.s1) + ((t.s2,) if opt == "adam" else ())])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    W0, b0, W1, b1, w2, b2 = runs[0][:6]
    D, (h0, h1) = 2 * S_SMALL, HID_SMALL
    assert not W0[h0:].any() and not W0[:, D:].any() and not b0[h0:].any()
    assert not W1[h1:].any() and not W1[:, h0:].any() and not b1[h1:].any()
    assert not w2[h1:].any() and not b2[1:].any()
    live = gc.layout.views(gc.layout.live_mask())
    for vec in runs[0][6:]:
        for v, m in zip(gc.layout.views(vec.cpu()), live):
            assert v[m].any() and not v[~m].any()


def test_zero_rows_and_zero_norms_stay_finite():
    gc, expert, _ = _small("least_squares", "sgd")
    expert = expert.clone()
    expert[:] = 0                       # every sampled expert row is all-zero
    gc.expert_data, gc._expert_dev = expert, None
    m = _run(gc, [R.synthetic_rows(BS_SMALL, S_SMALL, 90, 0.7, -0.2)])[0]
    assert all(np.isfinite(float(v)) for v in m.values()) and m["gradient_penalty"] > 0
    gc.w3.zero_()                       # every |d out / d x| = 0: U = 0, no NaN
    m = _run(gc, [R.synthetic_rows(BS_SMALL, S_SMALL, 91, 0.7, -0.2)])[0]
    assert all(np.isfinite(float(v)) for v in m.values()) and m["gradient_penalty"] == 0.0
    assert all(bool(torch.isfinite(w).all()) for w in _dev_weights(gc))
    assert bool(torch.isfinite(gc._train.s1).all())


# ---- inference after training, the regularizer, checkpoints ---------------------------------

@pytest.mark.parametrize("gemm", ["f16x3", "bf16x6", "f32"])
def test_inference_follows_training(gemm):
    from amp_extensions_amd.costs import GAILCost
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 80 + k, 0.7, -0.2) for k in range(3)]
    gc, expert, args = _small("least_squares", "sgd", gemm=gemm)
    x = R.synthetic_rows(200, S_SMALL, 95, 0.6, 0.0)
    before = gc.get_costs(x).clone()
    _run(gc, mbs)
    after = gc.get_costs(x).clone()
    assert not torch.equal(before, after)
    fresh = GAILCost(expert, hidden_dims=list(HID_SMALL), seed=100, device=DEV, gemm=gemm)
    fresh.load_weights(gc.disc.state_dict())
    assert torch.equal(fresh.get_costs(x), after)
    assert torch.equal(fresh.disc_logits(x), gc.disc_logits(x))


def test_bonus_costs_follow_training():
    from amp_extensions_amd.costs import GAILCost
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 80 + k, 0.7, -0.2) for k in range(3)]
    gc, expert, _ = _small("least_squares", "sgd")
    _run(gc, mbs)
    fresh = GAILCost(expert, hidden_dims=list(HID_SMALL), seed=100, device=DEV)
    fresh.load_weights(gc.disc.state_dict())

    class Ens:   # a stand-in with the surface the cost reads
        threshold = 1.0

        def get_action_discrepancy(self, s, a):
            return torch.linspace(0, 1, s.shape[0], device=DEV)

    import amp_extensions_amd.costs as C
    real = C.device_discrepancy
    C.device_discrepancy = lambda ens, s, a: ens.get_action_discrepancy(s, a)
    try:
        x = R.synthetic_rows(150, S_SMALL, 96, 0.6, 0.0).to(DEV)
        s, s2, a = x[:, :S_SMALL], x[:, S_SMALL:], torch.zeros(150, 3, device=DEV)
        c1, i1 = gc.get_bonus_costs(s, a, Ens(), s2)
        c2, i2 = fresh.get_bonus_costs(s, a, Ens(), s2)
    finally:
        C.device_discrepancy = real
    assert torch.equal(c1, c2) and all(torch.equal(i1[k], i2[k]) for k in i1)


def test_regularizer_leaves_no_trace():
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 80 + k, 0.7, -0.2) for k in range(3)]
    out = []
    for reg in (0.0, 5.0):
        gc, _, _ = _small("least_squares", "sgd", reg_coef=reg)
        out.append((_run(gc, mbs), _dev_weights(gc)))
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    for m0, m5 in zip(out[0][0], out[1][0]):
        assert m0["regularizer_loss"] == 0.0 and m5["regularizer_loss"] > 0.0
        assert m5["total_disc_loss"] > m0["total_disc_loss"]
        for key in ("expert_disc_loss", "model_based_disc_loss", "gradient_penalty"):
            assert m0[key] == m5[key]
        assert torch.equal(m0["expert_acc"], m5["expert_acc"]) and torch.equal(m0["mb_acc"], m5["mb_acc"])


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_checkpoint_resume(opt):
    import copy
    mbs = [R.synthetic_rows(BS_SMALL, S_SMALL, 80 + k, 0.7, -0.2) for k in range(6)]
    straight, _, _ = _small("least_squares", opt)
    _run(straight, mbs)
    first, expert, _ = _small("least_squares", opt)
    _run(first, mbs[:3])
    ck = copy.deepcopy({"disc": first.disc.state_dict(), "opt": first.disc_opt.state_dict()})
    assert list(ck["disc"]) == list(R.KEYS) and sorted(ck["opt"]["state"]) == list(range(6))
    for j, key in enumerate(R.KEYS):
        for tk in ("momentum_buffer",) if opt == "sgd" else ("exp_avg", "exp_avg_sq"):
            assert ck["opt"]["state"][j][tk].shape == ck["disc"][key].shape
    second, _, _ = _small("least_squares", opt, seed=7)    # other weights, replaced by the checkpoint
    second.load_weights(ck["disc"], optimizer=ck["opt"])
    state = np.random.get_state()
    np.random.seed(3)
    for _ in range(3):                                       # the draws the first three steps consumed
        np.random.randint(0, 90, BS_SMALL)
    [second.update_disc(mb) for mb in mbs[3:]]
    np.random.set_state(state)
    assert all(torch.equal(a, b) for a, b in zip(_dev_weights(straight), _dev_weights(second)))
    for tk in ("momentum_buffer",) if opt == "sgd" else ("exp_avg", "exp_avg_sq", "step"):
        assert all(torch.equal(a, b) for a, b in zip(_dev_state(straight, tk), _dev_state(second, tk)))


# ---- the replay buffer and the refusals -----------------------------------------------------

def test_replay_buffer_on_device(g16):
    from amp_extensions_amd.datasets import AgentReplayBuffer
    _, adds, agent = R.g16_inputs()
    rb = AgentReplayBuffer(device=DEV, max_size=G["max_size"])
    with pytest.raises(Exception, match="Not possible to sample from empty dataset."):
        rb.sample(4)
    with pytest.raises(Exception, match="Not possible to select from empty dataset."):
        rb[0]
    want = None
    for i, (s, s2) in enumerate(adds):
        rb.add(*((s.to(DEV), s2.to(DEV)) if i % 2 else (s, s2)))
        rows = torch.cat([s, s2], 1)
        want = (rows if want is None else torch.cat([want, rows], 0))[-G["max_size"]:]
        assert len(rb) == want.shape[0]
        assert torch.equal(torch.cat([rb.states, rb.next_states], -1).cpu(), want)
    assert rb.ring.is_cuda and rb.head != 0
    np.random.seed(G["blocks"]["adam_ll"]["seed"])
    got = rb.sample(256)     # the first draw of G16's adam_ll block
    assert got.is_cuda and torch.equal(got.cpu(), agent[g16["adam_ll_idx_m"][0]])


def test_update_without_buffer_asserts():
    gc, _, _ = _small("least_squares", "sgd")
    with pytest.raises(AssertionError, match="need to sample from online buffer"):
        gc.update_disc(None)
    with pytest.raises(AssertionError, match="Cannot compute divergence"):
        gc.compute_chi2_distance()
    with pytest.raises(AssertionError, match="Cannot sample from nonexistent buffer"):
        gc.sample_from_online_buffer(4)
    np.random.seed(1)
    got = gc.sample_from_expert_data(5)
    np.random.seed(1)
    assert torch.equal(got, gc.expert_data[np.random.randint(0, 90, 5)])


def test_refusals_come_before_any_allocation():
    from amp_extensions_amd.costs import GAILCost
    expert = R.synthetic_rows(90, S_SMALL, 61, 0.5, 0.3)
    deep = GAILCost(expert, hidden_dims=[64, 32, 32], seed=100, device=DEV)
    mb = R.synthetic_rows(BS_SMALL, S_SMALL, 80, 0.7, -0.2)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match="two hidden layers"):
        deep.update_disc(mb)
    assert deep._train is None and torch.cuda.memory_allocated() == mem
    gc, _, _ = _small("least_squares", "sgd")
    mem2 = torch.cuda.memory_allocated()
    sd = gc.disc.state_dict()
    nest = torch.optim.SGD(gc.disc.parameters(), lr=1e-5, momentum=0.9, nesterov=True).state_dict()
    with pytest.raises(NotImplementedError, match="without Nesterov"):
        gc.load_weights(sd, optimizer=nest)
    decay = torch.optim.Adam(gc.disc.parameters(), lr=1e-3, weight_decay=0.1).state_dict()
    with pytest.raises(NotImplementedError, match="no weight decay"):
        gc.load_weights(sd, optimizer=decay)
    assert gc._train is None and torch.cuda.memory_allocated() == mem2
