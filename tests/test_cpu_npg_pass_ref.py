"""Pins tests/npg_pass_ref.py, the fp64 reference the device NPG pass is held to
(tests/test_gpu_npg_pass.py), and measures the allowance K it is held with.

  * the closed forms against fp64 torch autograd of the oracle's own building blocks
    (oracle/milo_ref.py: _policy_mean_ll, _mean_kl, the CPI surrogate) run in double -- every mode,
    the whole batch and a row sub-range -- within 1e-12 of the magnitude companion;
  * hand-worked cases: a one-unit scalar chain at N = S = A = 1 written out with math.tanh /
    math.exp in all three modes; the FVP log_std slots exactly zero; EVAL at new == old exactly
    (sum float32(adv), 0.0);
  * the allowance: the project's fp32 oracle evaluates every case of the device tests; its
    largest ratio to the reference, in the unit |x - ref| / (2^-24 mag), must stay within K / 4 and
    must equal the maxima recorded next to K, so the constants cannot drift.
"""
import math

import numpy as np
import pytest
import torch

import npg_pass_ref as P
from oracle import milo_ref as R

VPG, FVP, EVAL = P.VPG, P.FVP, P.EVAL


def _params64(flat, S, A, grad):
    return [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(grad) for t in P.unpack(flat, S, A)]


def _autograd(mode, d, r0, r1):
    """fp64 autograd of the oracle's expressions over rows [r0, r1), divisor N."""
    S, A, N = d["S"], d["A"], d["N"]
    obs = torch.from_numpy(d["obs"][r0:r1]).double()
    act = torch.from_numpy(d["act"][r0:r1]).double()
    adv = torch.from_numpy(d["adv"][r0:r1])
    old = _params64(d["theta"], S, A, False)
    if mode == EVAL:
        new = _params64(d["new"], S, A, False)
        mo, LLo = R._policy_mean_ll(old, obs, act, A)
        mn, LLn = R._policy_mean_ll(new, obs, act, A)
        n = r1 - r0
        return np.array([float((torch.exp(LLn - LLo) * adv).sum()),
                         float(R._mean_kl(mn, new[-1], mo, old[-1]) * n)])
    new = _params64(d["theta"], S, A, True)
    mo, LLo = R._policy_mean_ll(old, obs, act, A)
    mn, LLn = R._policy_mean_ll(new, obs, act, A)
    if mode == VPG:
        g = torch.autograd.grad((torch.exp(LLn - LLo) * adv).sum() / N, new)
        return np.concatenate([x.reshape(-1).numpy() for x in g])
    kl = R._mean_kl(mn, new[-1], mo, old[-1]) * ((r1 - r0) / N)
    g = torch.autograd.grad(kl, new, create_graph=True)
    v = torch.from_numpy(d["vec"].astype(np.float64))
    h = (torch.cat([x.reshape(-1) for x in g]) * v).sum()
    hv = np.concatenate([x.reshape(-1).numpy() for x in torch.autograd.grad(h, new)])
    hv[-A:] = 0.0  # the log_std block is the caller's (npg_ls_curvature)
    return hv


@pytest.mark.parametrize("mode", [VPG, FVP, EVAL])
@pytest.mark.parametrize("S,A,N,r0,r1", [(197, 36, 70, 0, 70), (197, 36, 70, 32, 64), (17, 5, 33, 32, 33),
                                         (256, 64, 17, 0, 17), (1, 1, 40, 3, 37)])
def test_reference_matches_fp64_autograd(mode, S, A, N, r0, r1):
    d = P.inputs(S, A, N)
    ref, mag = P.pass_ref(mode, S, A, d["theta"], d["obs"], d["act"], d["adv"], P.mode_vec(d, mode), N, r0, r1)
    x = _autograd(mode, d, r0, r1)
    assert ref.shape == mag.shape == x.shape
    assert (np.abs(x - ref) <= 1e-12 * mag).all(), float((np.abs(x - ref) / np.maximum(mag, 1e-300)).max())
    assert (mag >= np.abs(ref)).all()  # the companion bounds its value


def _scalar_params(w, b, u, c, q, dd, ls):
    """S = A = 1 parameters with one live unit per hidden layer (the other 31 stay at tanh(0) = 0)."""
    th = np.zeros(P.param_count(1, 1), np.float32)
    seg = {n: lo for n, lo, _ in P.segments(1, 1)}
    for name, v in (("W1", w), ("b1", b), ("W2", u), ("b2", c), ("W3", q), ("b3", dd), ("log_std", ls)):
        th[seg[name]] = v
    return th, seg


def test_hand_worked_scalar_chain():
    """N = S = A = 1: mean = q tanh(u tanh(w x + b) + c) + d, written out with scalars."""
    w, b, u, c, q, dd, ls = 1.0, 0.5, 2.0, -0.25, 0.5, 1.0, 0.0
    x, a, adv = 0.5, 3.0, 0.75
    th, seg = _scalar_params(w, b, u, c, q, dd, ls)
    h1 = math.tanh(w * x + b)
    h2 = math.tanh(u * h1 + c)
    m, sd = q * h2 + dd, math.exp(ls)
    z = (a - m) / sd
    obs, act = np.array([[x]], np.float32), np.array([[a]], np.float32)

    def chain(Dm):  # (gw, gb, gu, gc, gq, gd)
        D2 = Dm * q * (1 - h2 * h2)
        D1 = D2 * u * (1 - h1 * h1)
        return {"W1": D1 * x, "b1": D1, "W2": D2 * h1, "b2": D2, "W3": Dm * h2, "b3": Dm}

    def check(ref, want):
        exp = np.zeros_like(ref)
        for k, v in want.items():
            exp[seg[k]] = v
        np.testing.assert_allclose(ref, exp, rtol=1e-14, atol=0)

    ref, mag = P.pass_ref(VPG, 1, 1, th, obs, act, [adv], None)
    check(ref, dict(chain(adv * z / sd), log_std=adv * (z * z - 1)))
    assert mag[seg["log_std"]] == pytest.approx(adv * (z * z + 1), rel=1e-14)
    # the divisor is the pass's N, not the range's length
    ref4, _ = P.pass_ref(VPG, 1, 1, th, obs, act, [adv], None, N=4)
    np.testing.assert_allclose(ref4, ref / 4, rtol=1e-15)

    vw, vb, vu, vc, vq, vd = 0.5, -1.0, 0.25, 2.0, -0.5, 1.5
    tv, _ = _scalar_params(vw, vb, vu, vc, vq, vd, 3.0)  # the log_std tangent is not read
    dh1 = (vw * x + vb) * (1 - h1 * h1)
    dh2 = (vu * h1 + u * dh1 + vc) * (1 - h2 * h2)
    jm = vq * h2 + q * dh2 + vd
    ref, mag = P.pass_ref(FVP, 1, 1, th, obs, act, None, tv)
    check(ref, chain(jm * 2.0 / (2.0 * sd * sd + 1e-8)))
    assert ref[seg["log_std"]] == 0.0 and mag[seg["log_std"]] == 0.0

    wn, bn, un, cn, qn, dn, lsn = 0.75, 0.25, 1.5, 0.5, 1.0, 0.5, -0.5
    tn, _ = _scalar_params(wn, bn, un, cn, qn, dn, lsn)
    mn, sn = qn * math.tanh(un * math.tanh(wn * x + bn) + cn) + dn, math.exp(lsn)
    zn = (a - mn) / sn
    LR = math.exp(-0.5 * zn * zn + 0.5 * z * z + ls - lsn)
    kl = ((m - mn) ** 2 + sd * sd - sn * sn) / (2 * sn * sn + 1e-8) + lsn - ls
    ref, mag = P.pass_ref(EVAL, 1, 1, th, obs, act, [adv], tn)
    np.testing.assert_allclose(ref, [LR * adv, kl], rtol=1e-14)
    np.testing.assert_allclose(mag, [adv * LR * (1 + 0.5 * zn * zn + 0.5 * z * z + abs(ls - lsn)),
                                     ((m - mn) ** 2 + sd * sd + sn * sn) / (2 * sn * sn + 1e-8) + abs(lsn) + abs(ls)],
                               rtol=1e-14)


@pytest.mark.parametrize("S,A,N", [(197, 36, 70), (1, 1, 17), (256, 64, 17)])
def test_exact_cases(S, A, N):
    d = P.inputs(S, A, N)
    ref, mag = P.pass_ref(FVP, S, A, d["theta"], d["obs"], d["act"], None, d["vec"], N, 3, N)
    assert (ref[-A:] == 0.0).all() and (mag[-A:] == 0.0).all() and not np.signbit(ref[-A:]).any()
    assert (np.float32(d["adv_exact"]) == d["adv_exact"]).all()
    for r0, r1 in ((0, N), (5, N - 1)):
        ref, _ = P.pass_ref(EVAL, S, A, d["theta"], d["obs"], d["act"], d["adv_exact"], d["theta"], N, r0, r1)
        assert ref[0] == float(np.float32(d["adv_exact"][r0:r1]).astype(np.float64).sum()) and ref[1] == 0.0


def test_case_lists():
    assert len(P.SHAPE_CASES) == 13 and len(set(P.SHAPE_CASES)) == 13
    assert {(1, 1), (16, 16), (256, 64), (255, 49)} <= set(P.SHAPE_CASES)
    assert {s for s, _ in P.SHAPE_CASES} >= set(P._S_EDGE) and {a for _, a in P.SHAPE_CASES} >= set(P._A_EDGE)
    assert all(rpb % 32 == 0 and n <= 600 for rpb, n in P.BLOCK_CASES + P.SHAPE_RUNS)
    assert sum(hi - lo for _, lo, hi in P.segments(P.S1, P.A1)) == P.param_count(P.S1, P.A1)


def _oracle_ratios(S, A, N, r0, r1):
    """The fp32 oracle's ratios to the reference per mode on rows [r0, r1) as a batch of its own."""
    d = P.inputs(S, A, N)
    th, obs, act, adv = d["theta"], d["obs"][r0:r1].copy(), d["act"][r0:r1].copy(), d["adv"][r0:r1].copy()
    n = r1 - r0
    shapes = R.policy_param_shapes(S, A, (32, 32))
    out = {}
    ref, mag = P.pass_ref(VPG, S, A, th, obs, act, adv, None)
    out[VPG] = P.ratio(R.npg_vpg(th, shapes, obs, act, adv)[0], ref, mag)
    ref, mag = P.pass_ref(FVP, S, A, th, obs, act, None, d["vec"])
    hv = R.npg_hvp(th, shapes, obs, act, d["vec"], 0.0)
    out[FVP] = P.ratio(hv[:-A], ref[:-A], mag[:-A])
    ref, mag = P.pass_ref(EVAL, S, A, th, obs, act, adv, d["new"])
    surr, _ = R._cpi_surrogate(d["new"], th, shapes, obs, act, adv)
    obs_t, act_t = torch.from_numpy(obs), torch.from_numpy(act)
    new, old = R._unflatten(d["new"], shapes), R._unflatten(th, shapes)
    mo, _ = R._policy_mean_ll(old, obs_t, act_t, A)
    mn, _ = R._policy_mean_ll(new, obs_t, act_t, A)
    kl = R._mean_kl(mn, new[-1], mo, old[-1])
    out[EVAL] = P.ratio([float(surr.detach()) * n, float(kl) * n], ref, mag)
    return out


@pytest.fixture(scope="module")
def oracle_max():
    """{mode: [(max, case) over every case, (max, case) over the ranges of >= MANY_ROWS rows]}"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one summation order whatever the machine's core count
    try:
        worst = {m: [(0.0, None), (0.0, None)] for m in (VPG, FVP, EVAL)}
        for case in P.oracle_cases():
            many = case[4] - case[3] >= P.MANY_ROWS
            for m, r in _oracle_ratios(*case).items():
                for tier in ((0, 1) if many else (0,)):
                    if float(r.max()) > worst[m][tier][0]:
                        worst[m][tier] = (float(r.max()), case)
    finally:
        torch.set_num_threads(threads)
    for m, w in worst.items():
        print(f"oracle max ratio {P.MODE_NAMES[m]}: all cases {w[0][0]:.3f} at {w[0][1]}; "
              f">= {P.MANY_ROWS} rows {w[1][0]:.3f} at {w[1][1]} (S, A, N, r0, r1)")
    return worst


def test_oracle_within_quarter_of_allowance(oracle_max):
    for m, ((v, case), (v15, case15)) in oracle_max.items():
        assert np.isfinite(v) and v <= P.K[m] / 4.0, (P.MODE_NAMES[m], v, case)
        assert v15 <= P.K15[m] / 4.0, (P.MODE_NAMES[m], v15, case15)


def test_allowance_is_four_times_the_recorded_maxima():
    for m in (VPG, FVP, EVAL):
        assert P.K[m] == math.ceil(4.0 * P.ORACLE_MAX[m]) and P.K15[m] == math.ceil(4.0 * P.ORACLE_MAX15[m])
        assert P.K15[m] <= P.K[m]
        assert P.allowance(m, P.MANY_ROWS) == P.K15[m] and P.allowance(m, P.MANY_ROWS - 1) == P.K[m]
