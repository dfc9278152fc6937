"""The NPG planner as run.py builds it, on the device: the Fisher-vector pass over an index vector
(amx_npg_pass_idx / amx_npg_pass_cg_idx), the log-likelihood pass (amx_npg_ll), DeviceNPG's BC term,
subsampled solve and dist-info entries, and the drop-in amp_extensions_amd.npg.NPG.

Bit for bit, no tolerances: the indexed pass and solve against the plain entry points on the
materialised rows obs[idx]; the LL pass against amx_ppo_old_ll; repeatability.

Against the comparator tests/npgreg_ref.py and the reference's recorded run G23, the project's
existing bounds only (tests/test_gpu_npg.py, tests/test_gpu_ppo.py): 1e-4 of max for the VPG
gradient and a single indexed Fisher-vector product, 2e-3 of max for the CG solution and the
parameter change, rtol 1e-3 for surr_after, abs 1e-6 for surr_before.  tests/test_cpu_npgreg.py
asserts on the comparator that these checks bite (the BC term and the subsampling each move the
result by far more than the bound) and that the fp32 reference sits within a quarter of each.
Bounds of derived quantities, written out where they are used:
  * alpha = sqrt(step / vpg.npg) and kl_dist ~ delta' F delta / 2 follow the solution: 2e-3 and
    2 * 2e-3 relative;
  * a row's LL at equal parameters differs by fp32 rounding only: |LL| eps32 times the ~300
    roundings of one row's forward and sum, 60 * 6e-8 * 300 ~ 1e-3 absolute;
  * a row's LL_new and log lr move with the parameter change delta: |g_r . (delta - delta_ref)| <=
    |g_r|_1 * 2e-3 max|delta|, g_r the row's LL gradient (computed by the test), plus the above.
"""
import math

import numpy as np
import pytest
import torch

import npgreg_ref as G
from oracle import milo_ref as R
from test_gpu_bcfit import _MjrlMLP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make(S, A, params, **kw):
    import amp_extensions_amd as amx
    from amp_extensions_amd.npg import unpack_policy
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV)
    layers, ls = unpack_policy(params, S, A)
    return amx.DeviceNPG(ctx, layers, ls, normalized_step_size=G.STEP,
                         FIM_invert_args={"iters": G.CG_ITERS, "damping": G.DAMPING}, min_log_std=G.MIN_LOG_STD, **kw)


def policy_params(S, A, seed=100):
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    return pack_policy(*init_mlp_policy_params(S, A, (32, 32), seed=seed, init_log_std=-0.25))


def rows(npg, N, seed):
    rs = np.random.RandomState(seed)
    S, A = npg.S, npg.A
    return npg._inputs((0.5 * rs.randn(N, S)).astype(np.float32), rs.randn(N, A).astype(np.float32), rs.randn(N))


def index_vector(rs, N, M):
    """M rows of N with row 0, row N - 1 and a thrice-repeated row among them."""
    idx = rs.randint(0, N, size=M).astype(np.int32)
    idx[0], idx[1] = 0, N - 1
    idx[2] = idx[3] = idx[4]
    return torch.from_numpy(idx).to(DEV)


# ---- bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("S,A", [(11, 3), (111, 8), (197, 36), (256, 64)])
def test_indexed_pass_is_the_plain_pass_on_materialised_rows(S, A):
    """The four layer-1 depths; M = 300 (a ragged chunk and a ragged last block), 31 (one short
    chunk) and 1024; with and without the theta cache."""
    from amp_extensions_amd.npg import NPG_FVP, NPG_VPG
    N = 700
    npg = make(S, A, policy_params(S, A))
    o, a, adv = rows(npg, N, 3)
    hc = torch.full((N, 64), float("nan"), dtype=torch.float32, device=DEV)
    npg._pass(NPG_VPG, o, a, adv, None, hcache=hc)
    rs = np.random.RandomState(5)
    vec = torch.from_numpy(rs.randn(npg.P).astype(np.float32)).to(DEV)
    for M in (300, 31, 1024):
        idx = index_vector(rs, N, M)
        li = idx.long()
        om, am = o[li].contiguous(), a[li].contiguous()
        for cache in (False, True):
            ref = npg._pass(NPG_FVP, om, am, None, vec, hcache=hc[li].contiguous() if cache else None,
                            reduce=False).clone()
            got = npg._pass_idx(o, idx, vec, hcache=hc if cache else None).clone()
            assert ref.shape == got.shape == (math.ceil(M / npg._rows_per_block(M)), npg.P)
            assert torch.equal(ref, got), (M, cache, float((ref - got).abs().max()))
        # the public product: the reduced pass, the log_std curvature and the damping
        hv = npg.HVP(o, a, vec, idx=idx)
        assert torch.equal(hv, npg.HVP(om, am, vec))


def solve_on_materialised_rows(npg, o, hc, b, idx, tol):
    """cg_solve's unfolded form from public entry points: amx_npg_pass_ex gated on p32 over the
    materialised rows of each iteration, then amx_npg_cg_tail."""
    from amp_extensions_amd.npg import NPG_FVP
    c, lib, P, A = npg.ctx, npg.ctx.lib, npg.P, npg.A
    x, r, p, r2 = (torch.empty(P, dtype=torch.float64, device=DEV) for _ in range(4))
    p32 = torch.empty(P, dtype=torch.float32, device=DEV)
    st, st2 = (torch.empty(2, dtype=torch.float64, device=DEV) for _ in range(2))
    curv = torch.empty(A, dtype=torch.float64, device=DEV)
    work = torch.empty(int(lib.amx_npg_cg_tail_work(P)), dtype=torch.float64, device=DEV)
    assert lib.amx_npg_cg_init_ls(c.h, P, A, npg.theta.data_ptr(), curv.data_ptr(), b.data_ptr(), x.data_ptr(),
                                  r.data_ptr(), p.data_ptr(), p32.data_ptr(), st.data_ptr(), c.stream) == 0
    for it in range(npg.cg_iters):
        li = idx[it].long()
        om = o[li].contiguous()
        part = npg._pass(NPG_FVP, om, om, None, p32, gate=st, hcache=hc[li].contiguous(), reduce=False)
        assert lib.amx_npg_cg_tail(c.h, part.data_ptr(), part.shape[0], P, A, curv.data_ptr(), npg.damping, tol,
                                   x.data_ptr(), r.data_ptr(), r2.data_ptr(), p.data_ptr(), p32.data_ptr(),
                                   st.data_ptr(), st2.data_ptr(), work.data_ptr(), c.stream) == 0
        r, r2, st, st2 = r2, r, st2, st
    torch.cuda.synchronize()
    return x.cpu().numpy()


def rr_history(npg, o, a, b, idx, steps):
    """r.r after each CG step, from a numpy CG with the device's indexed product as f_Ax."""
    bn = b.cpu().numpy()
    r_, p_ = bn.copy(), bn.copy()
    hist = [float(bn @ bn)]
    for it in range(steps):
        z = npg.HVP(o, a, p_, idx=idx[it]).cpu().numpy()
        v = hist[-1] / (p_ @ z)
        r_ = r_ - v * z
        nr = float(r_ @ r_)
        p_ = r_ + nr / hist[-1] * p_
        hist.append(nr)
    return hist


def stop_tol(hist):
    """A residual_tol first reached at the last step of `hist` (r.r after 0, 1, ... steps), placed
    as test_npg_cg_fold_bit_identical places it.  A Fisher on other rows every iteration does not
    shrink r.r monotonically, so the earlier steps are all checked."""
    assert hist[-1] < min(hist[1:-1])
    return float(np.sqrt(hist[-1] * min(hist[1:-1])))


@pytest.mark.parametrize("iters,stop_at", [(1, None), (2, None), (10, None), (10, 3)])
def test_indexed_solve_is_the_plain_solve_on_materialised_rows(iters, stop_at):
    """cg_solve with an index table, CG step folded into the next pass or not, against the
    test-side loop on materialised rows: the same x bit for bit, and the count of products taken
    (with the stop at iteration 3 placed as test_npg_cg_fold_bit_identical places it)."""
    from amp_extensions_amd.npg import NPG_VPG
    S, A, N, M = 197, 36, 3000, 1500
    npg = make(S, A, policy_params(S, A))
    npg.cg_iters = iters
    o, a, adv = rows(npg, N, 13)
    hc = npg._hcache(N)
    b = npg._pass(NPG_VPG, o, a, adv, None, hcache=hc).clone()
    rs = np.random.RandomState(17)
    idx = torch.stack([index_vector(rs, N, M) for _ in range(iters)]).contiguous()
    tol = 0.0
    if stop_at is not None:
        hist = rr_history(npg, o, a, b, idx, stop_at)
        tol = stop_tol(hist)
    x_ref = solve_on_materialised_rows(npg, o, hc, b, idx, tol)
    for fold in (False, True):
        npg.cg_fold, npg.residual_tol = fold, tol
        count = torch.zeros(1, dtype=torch.float64, device=DEV)
        x = npg.cg_solve(o, a, b, hcache=hc, idx=idx, count=count).cpu().numpy()
        assert np.array_equal(x, x_ref), (fold, np.abs(x - x_ref).max())
        assert int(count.item()) == (iters if stop_at is None else stop_at)
    if stop_at is not None:  # the stop took effect after `stop_at` steps
        npg.cg_iters = stop_at
        assert np.array_equal(x_ref, solve_on_materialised_rows(npg, o, hc, b, idx, 0.0))


@pytest.mark.parametrize("S,A,N", [(197, 36, 1000), (11, 3, 130)])
def test_ll_pass(S, A, N):
    """amx_npg_ll: the rows' LL are amx_ppo_old_ll's bits, so equal parameters give lr == 1 on
    every row; the block partials add up to the fp64 sum of the row values (exactly: a few
    thousand fp32 values of one size, nothing rounds in fp64); the mean is the policy's."""
    from amp_extensions_amd import _native as N_
    p0 = policy_params(S, A)
    npg = make(S, A, p0)
    o, a, _ = rows(npg, N, 21)
    c = npg.ctx
    tot, ll, mean = npg.log_likelihood(o, a, rows=True)
    _, ll2, _ = npg.log_likelihood(o, a, npg.theta.clone(), rows=True)
    assert bool((torch.exp(ll2 - ll) == 1.0).all())
    ll_ppo = torch.empty(N, dtype=torch.float32, device=DEV)
    N_.check(c.lib.amx_ppo_old_ll(c.h, N, o.data_ptr(), o.stride(0), a.data_ptr(), a.stride(0), npg.theta.data_ptr(),
                                  ll_ppo.data_ptr(), c.stream), "amx_ppo_old_ll")
    assert torch.equal(ll, ll_ppo)
    assert float(tot.item()) == math.fsum(ll.cpu().double().tolist())
    only = npg.log_likelihood(o, a)  # without the per-row outputs
    assert torch.equal(only, tot)
    ref = G.policy_mean(p0, S, A, o.cpu().numpy())
    assert np.abs(mean.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    ll_ref = G._ll32(p0, R.policy_param_shapes(S, A), o.cpu().numpy(), a.cpu().numpy()).numpy()
    assert np.abs(ll.cpu().numpy() - ll_ref).max() <= 1e-3


def update_case(npg, c, bc, idx=None, **kw):
    out = npg.train_from_arrays(c["obs"], c["act"], c["adv"], bc=bc, idx=idx, **kw)
    torch.cuda.synchronize()
    return out


def test_updates_repeat_and_the_plain_path_is_unchanged():
    S, A, n = 111, 8, 2048
    c = G.case_inputs(S, A, n)
    bc = (c["expert_obs"], c["expert_act"], G.REG_COEFF)
    idx = np.asarray(G.draws(3, n, 0.5), dtype=np.int32)
    runs = []
    for _ in range(2):
        npg = make(S, A, c["p0"], hvp_sample_frac=0.5)
        out = update_case(npg, c, bc, idx=idx, dist_info=True)
        runs.append([out[k].cpu().numpy() for k in ("vpg_grad", "npg_grad", "lr")] + [npg.get_param_values()] +
                    [np.float64(out[k]) for k in ("alpha", "surr_before", "surr_after", "kl_dist")])
    for u, v in zip(*runs):
        assert np.array_equal(u, v)
    # frac = 1, no BC, no dist-info: today's path, and the extended path with nothing to add
    plain, ext = make(S, A, c["p0"], hvp_sample_frac=1.0), make(S, A, c["p0"])
    ext.eval_before = True
    o0, o1 = update_case(plain, c, None), update_case(ext, c, None)
    assert o0["surr_before"] == 0.0 and "lr" not in o0 and "hvp_products" not in o0
    for k in ("vpg_grad", "npg_grad", "advantages"):
        assert torch.equal(o0[k], o1[k])
    for k in ("alpha", "delta", "surr_after", "kl_dist"):
        assert o0[k] == o1[k]
    assert torch.equal(plain.theta, ext.theta)
    assert abs(o1["surr_before"]) <= G.ATOL_SURR_BEFORE  # the mean of whitened advantages


# ---- against the comparator ----------------------------------------------------------------------

@pytest.mark.parametrize("S,A,n,frac,with_bc", G.CASES)
def test_update_vs_comparator(S, A, n, frac, with_bc):
    c, ref = G.case_inputs(S, A, n), G.case_ref(S, A, n, frac, with_bc)
    bc = (c["expert_obs"], c["expert_act"], G.REG_COEFF) if with_bc else None
    npg = make(S, A, c["p0"], hvp_sample_frac=frac)
    shapes = R.policy_param_shapes(S, A)
    v = np.random.RandomState(9).randn(c["p0"].size)
    hv = npg.HVP(c["obs"], c["act"], v, idx=ref["idx"][0]).cpu().numpy()
    hv_ref = R.npg_hvp(c["p0"], shapes, c["obs"][ref["idx"][0]], c["act"][ref["idx"][0]], v, G.DAMPING)
    assert G.maxrel(hv, hv_ref) <= G.TOL_VPG
    assert G.maxrel(npg.flat_vpg(c["obs"], c["act"], c["adv_w"], bc=bc).cpu().numpy(), ref["vpg"]) <= G.TOL_VPG
    np.random.seed(G.DRAW_SEED)
    out = update_case(npg, c, bc)
    assert G.maxrel(out["vpg_grad"].cpu().numpy(), ref["vpg"]) <= G.TOL_VPG
    assert G.maxrel(out["npg_grad"].cpu().numpy(), ref["npg"]) <= G.TOL_NPG
    p0 = c["p0"].astype(np.float64)
    assert G.maxrel(npg.get_param_values() - p0, ref["params1"] - p0) <= G.TOL_NPG
    np.testing.assert_allclose(out["surr_after"], ref["surr_after"], rtol=G.RTOL_SURR)
    assert abs(out["surr_before"] - ref["surr_before"]) <= G.ATOL_SURR_BEFORE
    # ten products, ten draws: numpy's stream is where the reference's loop leaves it
    rs = np.random.RandomState(G.DRAW_SEED)
    G.draws(rs, n, frac)
    st, end = np.random.get_state(), rs.get_state()
    assert out["hvp_products"] == G.CG_ITERS and st[2] == end[2] and np.array_equal(st[1], end[1])


def row_ll_grad_l1(flat, S, A, obs, act):
    """|d LL_r / d theta|_1 per row (fp64 autograd)."""
    shapes = R.policy_param_shapes(S, A)
    p = G._unflat64(np.asarray(flat, np.float64), shapes, grad=True)
    o, a = (torch.from_numpy(np.asarray(x, np.float32)).double() for x in (obs, act))
    _, ll = R._policy_mean_ll(p, o, a, A)
    out = []
    for r in range(len(ll)):
        g = torch.autograd.grad(ll[r], p, retain_graph=True)
        out.append(sum(float(x.abs().sum()) for x in g))
    return np.asarray(out)


def test_g23_through_the_drop_in(golden):
    """The reference's recorded run (two consecutive train_from_paths calls, hvp_sample_frac 0.5,
    bc_args, numpy seeded) through amp_extensions_amd.npg.NPG: every recorded infos value, the
    policy's parameters after each call, running_score and numpy's generator state."""
    import amp_extensions_amd as amx
    g = golden("g23_npg_reg.npz")
    S, A = 226, 28
    pol = _MjrlMLP(S, A, seed=int(g["model_seed"]), init_log_std=float(g["init_log_std"]),
                   min_log_std=float(g["min_log_std"]))
    pol.set_param_values(g["params0"].copy(), set_new=True, set_old=True)
    bc_args = {"flag": True, "expert_paths": {"observations": g["expert_obs"].astype(np.float64),
                                              "actions": g["expert_act"]}, "reg_coeff": float(g["reg_coeff"])}
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV)
    agent = amx.NPG(None, pol, None, normalized_step_size=float(g["step"]),
                    FIM_invert_args={"iters": int(g["cg_iters"]), "damping": float(g["damping"])},
                    hvp_sample_frac=float(g["frac"]), seed=100, save_logs=True, bc_args=bc_args, ctx=ctx)
    ends = np.cumsum(g["lengths"])
    np.random.seed(int(g["numpy_seed"]))
    score, params = None, g["params0"].astype(np.float64)
    for k in range(2):
        rec = {key[4:]: g[key] for key in g.files if key.startswith(f"c{k}__")}
        paths = [dict(observations=rec["observations"][e - l:e].astype(np.float64), actions=rec["actions"][e - l:e],
                      advantages=rec["advantages"][e - l:e], rewards=rec["rewards"][e - l:e])
                 for l, e in zip(g["lengths"], ends)]
        infos = {}
        stats = agent.train_from_paths(paths, infos)
        torch.cuda.synchronize()
        returns = [sum(p["rewards"]) for p in paths]
        assert stats == [np.mean(returns), np.std(returns), np.amin(returns), np.amax(returns)]
        score = np.mean(returns) if score is None else 0.9 * score + 0.1 * np.mean(returns)
        assert infos["running_score"] == agent.running_score == score
        np.testing.assert_allclose(score, float(rec["running_score"]), rtol=1e-12)
        np.testing.assert_allclose(infos["advantages"], rec["adv_whitened"], rtol=1e-12, atol=1e-15)
        assert infos["vpg_grad"].dtype == infos["npg_grad"].dtype == np.float32
        assert G.maxrel(infos["vpg_grad"], rec["vpg"]) <= G.TOL_VPG
        assert G.maxrel(infos["npg_grad"], rec["npg"]) <= G.TOL_NPG
        np.testing.assert_allclose(infos["alpha"], float(rec["alpha"]), rtol=G.TOL_NPG)
        assert abs(float(infos["surr_before"]) - float(rec["surr_before"])) <= G.ATOL_SURR_BEFORE
        np.testing.assert_allclose(infos["surr_after"], float(rec["surr_after"]), rtol=G.RTOL_SURR)
        np.testing.assert_allclose(infos["surr_improvement"], float(rec["surr_after"]) - float(rec["surr_before"]),
                                   rtol=G.RTOL_SURR, atol=G.ATOL_SURR_BEFORE)
        np.testing.assert_allclose(infos["kl_dist"], float(rec["kl_dist"]), rtol=2 * G.TOL_NPG)
        new = pol.get_param_values().astype(np.float64)
        assert G.maxrel(new - params, rec["params"].astype(np.float64) - params) <= G.TOL_NPG
        old = np.concatenate([p.data.numpy().ravel() for p in pol.old_params])
        assert np.array_equal(old, pol.get_param_values())
        assert (new[-A:] >= float(g["min_log_std"])).all()
        # the dist-info entries: [LL, mean, log_std] of the old and the new parameters, and lr
        ll_old, ll_new, lr = infos["old_dist_info"][0].numpy(), infos["new_dist_info"][0].numpy(), infos["lr"].numpy()
        assert infos["old_dist_info"][1].shape == (len(ll_old), A) and infos["new_dist_info"][2].shape == (A,)
        assert np.array_equal(infos["new_dist_info"][2].numpy(), pol.get_param_values()[-A:])
        ll_tol = 1e-3
        assert np.abs(ll_old - rec["ll_old"]).max() <= ll_tol
        delta = rec["params"].astype(np.float64) - params
        bound = row_ll_grad_l1(rec["params"], S, A, rec["observations"], rec["actions"]) * G.TOL_NPG * np.abs(delta).max()
        assert (np.abs(ll_new - rec["ll_new"]) <= bound + ll_tol).all()
        assert (np.abs(np.log(lr) - np.log(rec["lr"])) <= bound + 2 * ll_tol).all()
        for key in ("alpha", "delta", "time_vpg", "time_npg", "kl_dist", "surr_improvement", "running_score"):
            assert len(agent.logger.log[key]) == k + 1
        params = new
    st = np.random.get_state()
    assert st[2] == int(g["rng_pos"]) and np.array_equal(st[1], g["rng_keys"])


def test_early_stop_leaves_numpy_after_three_draws():
    """A residual_tol the solve reaches at its third product: three index vectors are consumed and
    numpy's generator is left after exactly three draws, where the reference's loop breaks."""
    from amp_extensions_amd.npg import NPG_VPG
    S, A, n, frac, seed = 111, 8, 2048, 0.5, 41
    c = G.case_inputs(S, A, n)
    npg = make(S, A, c["p0"], hvp_sample_frac=frac)
    o, a, adv = npg._inputs(c["obs"], c["act"], c["adv_w"])
    b = npg._pass(NPG_VPG, o, a, adv, None).clone()
    rs = np.random.RandomState(seed)
    idx = G.draws(rs, n, frac, 3)
    hist = rr_history(npg, o, a, b, [torch.from_numpy(i.astype(np.int32)).to(DEV) for i in idx], 3)
    npg.residual_tol = stop_tol(hist)
    np.random.seed(seed)
    out = npg.train_from_arrays(c["obs"], c["act"], c["adv_w"], whiten=False)
    st, end = np.random.get_state(), rs.get_state()
    assert out["hvp_products"] == 3 and st[2] == end[2] and np.array_equal(st[1], end[1])
    assert np.array_equal(np.random.choice(n, size=5), rs.choice(n, size=5))


def test_drop_in_refuses_old_parameters_that_differ():
    import amp_extensions_amd as amx
    S, A = 11, 3
    pol = _MjrlMLP(S, A, seed=3, min_log_std=-2.0)
    agent = amx.NPG(None, pol, None, normalized_step_size=0.1,
                    ctx=amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV))
    rs = np.random.RandomState(1)
    paths = [dict(observations=rs.randn(40, S), actions=rs.randn(40, A), advantages=rs.randn(40), rewards=rs.randn(40))]
    moved = pol.get_param_values() + np.float32(0.01)
    pol.set_param_values(moved, set_new=True, set_old=False)
    with pytest.raises(ValueError, match="old_params differ"):
        agent.train_from_paths(paths, {})
    pol.set_param_values(moved, set_new=True, set_old=True)
    infos = {}
    agent.train_from_paths(paths, infos)
    assert np.isfinite(infos["surr_after"]) and infos["lr"].shape == (40,)
