"""The CPU reference of the reward kernels (tests/cost_ref.py) against the oracle on real inputs,
and the properties its exactly summable operands promise: the same row dots in three fp64
summation orders, both clamp bounds cutting a good share of rows, and on the real cases the
share of rows that may deviate by one fp32 step."""
import numpy as np
import pytest
import torch

import cost_ref as C
from oracle import milo_ref as R

torch.set_num_threads(1)
S, A = 24, 6


def close(x, y, rtol=1e-6, atol=1e-7):  # test_oracle_golden.py's tolerance for these quantities
    x, y = np.asarray(x), np.asarray(y)
    if np.array_equal(x, y):
        return
    np.testing.assert_allclose(x, y, rtol=rtol, atol=atol)


def offline(n, seed):
    rs = np.random.RandomState(seed)
    s = 0.5 * rs.randn(n, S)
    return s, rs.randn(n, A), s + 0.05 * rs.randn(n, S)


@pytest.mark.parametrize("cost_range", [(-1.0, 0.0), (-0.002, 0.001), None])
def test_rewards_and_expert_cost_match_the_oracle(cost_range):
    es, _, es2 = offline(300, 0)
    expert = torch.from_numpy(np.concatenate([es, es2], 1)).float()
    lam, thr = 0.0025, 0.07
    c = R.RBFLinearCostRef(expert, feature_dim=256, cost_range=cost_range, bw_samples=2000, lambda_b=lam, seed=3)
    ps, pa, ps2 = offline(200, 1)
    rs = np.random.RandomState(5)
    dvals = torch.from_numpy(rs.uniform(0.0, 0.2, 200)).float()
    paths, o = [], 0
    for ln in (120, 80):
        paths.append({"observations": ps[o:o + ln], "next_observations": ps2[o:o + ln], "actions": pa[o:o + ln],
                      "rewards": np.zeros(ln), "disc": dvals[o:o + ln]})
        o += ln
    lut = {p["observations"][0, 0].astype(np.float32).item(): p["disc"] for p in paths}
    disc_fn = lambda st, ac: lut[st[0, 0].item()].clone()
    x = torch.from_numpy(np.concatenate([ps, ps2], 1)).float()
    phi = c.get_rep(x).numpy()
    if cost_range is not None:
        infos = R.relabel_mmd(paths, c, disc_fn, thr)
        ref_reward = np.concatenate([p["rewards"] for p in paths])
    else:
        infos = {"mb_mmd": c.fit_cost(x)}
        cost, _ = c.get_bonus_costs(torch.from_numpy(ps).float(), torch.from_numpy(pa).float(),
                                    lambda st, ac: dvals.clone(), thr, next_states=torch.from_numpy(ps2).float())
        ref_reward = -cost[:, 0].numpy()
    # the fit from the fp64 column sum
    msg = np.concatenate([phi.astype(np.float64).sum(0), [200.0]])
    w, mmd, _, _, _ = C.mmd_fit(msg, 0.0, c.phi_e.numpy())
    close(w, c.w.numpy(), atol=1e-7)
    close(mmd, infos["mb_mmd"])
    assert C.same_bits(w, C.mmd_fit(msg[:-1], 200.0, c.phi_e.numpy())[0])
    # rows scored with the oracle's own witness
    cmin, cmax = cost_range if cost_range is not None else (0.0, 0.0)
    cost, info = c.get_bonus_costs(torch.from_numpy(ps).float(), torch.from_numpy(pa).float(),
                                   lambda st, ac: dvals.clone(), thr, next_states=torch.from_numpy(ps2).float())
    reward, ipm, wb, near = C.rewards(phi, c.w.numpy(), dvals.numpy(), thr, lam, cmin, cmax, cost_range is not None)
    close(reward, ref_reward)
    close(reward, -cost[:, 0].numpy())
    close(ipm, info["ipm"][:, 0].numpy())
    close(wb, info["bonus"][:, 0].numpy())
    if cost_range is not None:
        tot, mean, terms, _, _ = C.expert_cost(c.expert_rep.numpy(), c.w.numpy(), lam, cmin, cmax)
        close(mean, c.get_expert_cost().item())
        close(tot / 300, terms.astype(np.float64).mean(), rtol=1e-12)


@pytest.mark.parametrize("loss", [0, 1])
def test_disc_reward_matches_the_oracle(loss):
    wts = R.init_disc_weights(2 * S, (64, 32), 1, 7)
    ps, pa, ps2 = offline(96, 4)
    ss = torch.from_numpy(np.concatenate([ps, ps2], 1)).float()
    with torch.no_grad():
        h = ss
        for W, b in wts[:-1]:
            h = torch.relu(torch.nn.functional.linear(h, W, b))
    w3, b3 = wts[-1][0][0].numpy(), float(wts[-1][1][0])
    rew, D, _ = C.disc_reward(h.numpy(), w3, b3, loss, None, 0.0025)
    close(D, R.disc_forward(wts, ss)[:, 0].numpy())
    costs = R.gail_ls_costs if loss == 0 else R.gail_ll_costs
    close(-rew, costs(wts, ss)[:, 0].numpy())
    dvals = torch.from_numpy(np.random.RandomState(2).uniform(0, 0.2, 96)).float()
    cost, _ = R.gail_bonus_costs(wts, torch.from_numpy(ps).float(), torch.from_numpy(pa).float(),
                                 torch.from_numpy(ps2).float(), lambda s, a: dvals.clone(), 0.0025,
                                 disc_loss_type="least_squares" if loss == 0 else "log_likelihood")
    reward, _, _ = C.disc_reward(h.numpy(), w3, b3, loss, dvals.numpy(), 0.0025)
    close(-reward, cost[:, 0].numpy())


def test_ll_formula_is_logsigmoid():
    D = np.array(C.HEAD_LOGITS + [3.0, -3.0, 0.5], np.float32)
    ref = -torch.nn.functional.logsigmoid(torch.from_numpy(D).double()).numpy()
    np.testing.assert_allclose(C.ll_reward_ld(D).astype(np.float64), ref, rtol=1e-14, atol=0)
    close(C.ll_reward_f32(D), ref.astype(np.float32))


def _check_exact_rows(rows, w):
    fwd = C.row_dots_f64(rows, w, "forward")
    assert np.array_equal(fwd, C.row_dots_f64(rows, w, "reversed"))
    assert np.array_equal(fwd, C.row_dots_f64(rows, w, "lanes"))
    d, lo, hi, near = C.dot32(rows, w)
    # exact in fp32 too; the worst-case bound can only straddle a rounding at a dot of exactly 0
    assert np.array_equal(d.astype(np.float64), fwd) and not near[fwd != 0].any()
    return fwd


def _check_shares(d):
    for share in ((d < C.C_MIN).mean(), ((d >= C.C_MIN) & (d <= C.C_MAX)).mean(), (d > C.C_MAX).mean()):
        assert share >= 0.10, share


@pytest.mark.parametrize("F", C.REWARD_F)
def test_exact_reward_cases_are_order_free(F):
    case = C.reward_case("exact", F)
    w, mmd, lo, hi, near = C.mmd_fit(case["msg"], 0.0, case["phi_e"])
    assert not near and np.abs(case["phi"] * 64).max() <= 63 and np.all(case["phi"] * 64 == np.rint(case["phi"] * 64))
    assert np.all(w * 64 == np.rint(w * 64)) and mmd == np.float32(np.sum(w.astype(np.float64) ** 2))
    _check_shares(_check_exact_rows(case["phi"], w))
    assert (case["disc"] < C.THR).mean() > 0.1 and (case["disc"] > C.THR).mean() > 0.1


@pytest.mark.parametrize("F,n_e", C.EXPERT_CASES)
def test_exact_expert_cases_are_order_free(F, n_e):
    case = C.expert_case("exact", F, n_e)
    w = C.witness(case)
    _check_exact_rows(case["erows"][:512], w)  # the rows are drawn alike: the first 512 stand for all
    d = C.dot32(case["erows"], w)[0]
    assert np.all(d * 4096 == np.rint(d * 4096)) and np.abs(d).max() < 4
    if n_e >= 63:
        _check_shares(d)
    tot, mean, terms, near, bound = C.expert_cost(case["erows"], w, C.LAM, C.C_MIN, C.C_MAX)
    assert np.all(terms * 4096 == np.rint(terms * 4096)) and terms.min() >= -1 and terms.max() <= 0
    t64 = terms.astype(np.float64)
    assert tot == np.sum(t64) == np.sum(t64[::-1]) == C.expert_partials(terms).sum()


@pytest.mark.parametrize("Hd", C.HEAD_HD)
def test_exact_head_cases_are_order_free(Hd):
    case = C.make_head("exact", Hd, C.HEAD_ROWS, 0)
    d = _check_exact_rows(case["h"], case["w3"])
    assert np.array_equal(d[:len(C.HEAD_LOGITS)].astype(np.float32), np.array(C.HEAD_LOGITS, np.float32))


def _near_share(rows, w):
    d, lo, hi, near = C.dot32(rows, w)
    assert np.isfinite(d).all() and np.all(lo <= d) and np.all(d <= hi) and np.abs(d).max() > 0
    return near.mean()


@pytest.mark.parametrize("F", C.REWARD_F)
def test_real_reward_cases_near_share(F):
    case = C.reward_case("real", F)
    assert _near_share(case["phi"], C.witness(case)) <= 0.01


@pytest.mark.parametrize("F,n_e", C.EXPERT_CASES)
def test_real_expert_cases_near_share(F, n_e):
    case = C.expert_case("real", F, n_e)
    assert _near_share(case["erows"], C.witness(case)) <= 0.01


@pytest.mark.parametrize("Hd", C.HEAD_HD)
def test_real_head_cases_near_share(Hd):
    case = C.make_head("real", Hd, C.HEAD_ROWS, 0)
    assert _near_share(case["h"], case["w3"]) <= 0.01


def test_near_flags_a_rounding_boundary():
    """A dot one part in 2^40 off an fp32 midpoint is flagged; the same dot at the grid point is not."""
    w = np.ones(128, np.float32)
    row = np.zeros((2, 128), np.float32)
    row[0, 0], row[0, 1], row[0, 2] = 1.0, 2.0 ** -24, 2.0 ** -47   # 1 + half an ulp (+ a little)
    row[1, 0] = 1.0
    d, lo, hi, near = C.dot32(row, w)
    assert near.tolist() == [True, False] and lo[0] == 1.0 and hi[0] == np.float32(1.0 + 2.0 ** -23)


def test_colsum_and_cost_rows():
    parts = C.int_parts(65, 16, 0)
    assert np.array_equal(C.colsum(parts, 16), parts.sum(0)) and np.array_equal(C.colsum(parts[:0], 16), np.zeros(16))
    x0, x2 = np.arange(10.0).reshape(2, 5) + 1e-9, np.arange(8.0).reshape(2, 4)
    out = C.cost_rows([x0, None, x2], [3, 0, 2], 8)
    assert out.dtype == np.float32 and np.array_equal(out[:, 5:], np.zeros((2, 3)))
    assert np.array_equal(out[:, :3], x0[:, :3].astype(np.float32)) and np.array_equal(out[:, 3:5], x2[:, :2])
