"""tests/npg_cg_ref.py pinned on the CPU: the reference the solve-half kernels are held to
(tests/test_gpu_npg_cg.py) solves a linear system, follows cg_solve.py line by line, breaks where
the oracle's loop breaks, and reproduces the oracle's step on the recorded G11 update."""
import numpy as np
import pytest

import npg_cg_ref as C
from npg_cg_cases import operands, reference
from oracle import milo_ref as R


def spd(n=40, cond=10.0, seed=0):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(n, n))
    return (q * np.geomspace(1.0, cond, n)) @ q.T, rs.randn(n)


def iterate(M, b, iters, tol=0.0, A=3):
    """cg_step driven as the kernels are: h = M p, no curvature, no damping.  Returns (x, r.r after
    every step taken, the number of products)."""
    s = C.cg_init(b)
    x, r, p, p32, state = s["x"], s["r"], s["p"], s["p32"], s["state"]
    hist, calls = [], 0
    for _ in range(iters):
        if state[1] != 0.0:
            calls += 1
        o = C.cg_step(M @ p, np.zeros(A), 0.0, tol, x, r, p, p32, state, A)
        x, r, p, p32, state = o["x"], o["r"], o["p"], o["p32"], o["state"]
        if o["live"]:
            hist.append(o["rr"])
    return x, hist, calls


def test_two_prod_sums_match_rational_arithmetic():
    rs = np.random.RandomState(1)
    for n in (1, 2, 63, 700):
        a, b = rs.randn(n) * np.exp(rs.randn(n) * 8), rs.randn(n)
        p, e = C.two_prod(a, b)
        for i in range(min(n, 50)):
            assert C.Fraction(p[i]) + C.Fraction(e[i]) == C.Fraction(a[i]) * C.Fraction(b[i])
        assert C.dot(a, b)[0] == C.dot_fraction(a, b)
    # a sum whose float64 evaluation loses everything
    assert C.dot([1e16, 1.0, -1e16], [1.0, 1.0, 1.0])[0] == 1.0
    assert C.fma(3.0, 1.0 + 2.0 ** -52, -3.0) == 3.0 * 2.0 ** -52


def test_cg_step_solves_spd_system():
    M, b = spd()
    assert np.linalg.cond(M) <= 100.0
    x, hist, _ = iterate(M, b, 40)
    want = np.linalg.solve(M, b)
    assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max(), np.abs(x - want).max()
    assert hist[-1] < 1e-20 * hist[0]


def test_cg_step_history_matches_cg_solve_restated():
    """cg_solve.py:3-23 restated in float64 numpy: the same r.r after every iteration to a few ulp
    (the restatement's dots round every product and partial sum, the reference's only the total)."""
    M, b = spd(seed=2)
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rdotr, want = r.dot(r), []
    for _ in range(12):
        z = M.dot(p)
        v = rdotr / p.dot(z)
        x += v * p
        r -= v * z
        newrdotr = r.dot(r)
        mu = newrdotr / rdotr
        p = r + mu * p
        rdotr = newrdotr
        want.append(rdotr)
    xr, hist, _ = iterate(M, b, 12)
    # 40-term float64 dots are good to ~40 * 2^-53 relative, a handful of ulp per iteration; the
    # recurrence on a condition-10 system carries each iteration's into the later r.r values, not
    # amplified: 8 ulp for the first two, 128 ulp over all twelve
    np.testing.assert_allclose(hist[:2], want[:2], rtol=8 * 2.0 ** -52)
    np.testing.assert_allclose(hist, want, rtol=128 * 2.0 ** -52)
    np.testing.assert_allclose(xr, x, rtol=0, atol=1e-12 * np.abs(x).max())


def test_cg_step_early_stop_breaks_where_the_oracle_breaks():
    M, b = spd(seed=3)
    _, hist, _ = iterate(M, b, 10)
    tol = float(np.sqrt(hist[3] * hist[4]))  # reached by the fifth step
    calls = []

    def f_Ax(p):
        calls.append(1)
        return M @ p

    want = R.cg_solve(f_Ax, b, cg_iters=10, residual_tol=tol)
    x, h2, n = iterate(M, b, 10, tol=tol)
    assert n == len(calls) == len(h2) == 5
    np.testing.assert_allclose(x, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # the contract's z: the curvature is added from float32(p) on the last A only, damping everywhere
    p = np.arange(1.0, 7.0)
    z, mag = C.cg_z(2.0 * p, np.array([0.25, 0.5]), 0.5, p, (p + 64.0).astype(np.float32), 2)
    np.testing.assert_array_equal(z, 2.5 * p + np.array([0, 0, 0, 0, 0.25 * 69, 0.5 * 70]))
    np.testing.assert_array_equal(mag, z)


def test_step_and_curvature_match_oracle_on_g11(golden):
    """apply_step on G11's recorded vpg / npg gives the recorded parameters at test_gpu_npg.py's
    tolerance for them (2e-3 of the largest move; the oracle forms alpha from float32 vectors), and
    ls_curvature is the log_std diagonal of the oracle's Fisher-vector product at that test's 1e-4."""
    g = golden("g11_npg.npz")
    S, A = 226, 28
    p0 = g["params0"]
    o = C.apply_step(g["vpg"], g["npg"], p0, 0, 0.0, float(g["step"]), float(g["min_log_std"]), A)
    move, want = o["new"].astype(np.float64) - p0, g["params1"].astype(np.float64) - p0
    assert np.abs(move - want).max() <= 2e-3 * np.abs(want).max()
    assert (o["new"][-A:] >= np.float32(g["min_log_std"])).all()
    assert abs(o["scal"][0] ** 2 * o["scal"][2] - float(g["step"])) <= 1e-12
    # const_learn_rate: n_step_size = alpha^2 gdot
    oa = C.apply_step(g["vpg"], g["npg"], p0, 1, 0.5, 0.0, float(g["min_log_std"]), A)
    assert oa["scal"][0] == 0.5 and oa["scal"][1] == 0.25 * oa["scal"][2] == 0.25 * o["scal"][2]
    # the clamp, NaN kept
    t = C.clamp_log_std(np.array([-9.0, -9.0, np.nan, -1.0], np.float32), -2.0, 3)
    np.testing.assert_array_equal(t, np.array([-9.0, -2.0, np.nan, -1.0], np.float32))
    # the Fisher's log_std block is diagonal: with v = 1 on it the product there is curv + damping
    shapes = R.policy_param_shapes(S, A, (32, 32))
    v = np.zeros(p0.size, np.float32)
    v[-A:] = 1.0
    hv = R.npg_hvp(p0, shapes, g["observations"].astype(np.float64), g["actions"], v, float(g["damping"]))
    curv, mag = C.ls_curvature(p0[-A:])
    want = hv[-A:].astype(np.float64) - float(g["damping"])
    assert np.abs(curv - want).max() <= 1e-4 * np.abs(want).max(), np.abs(curv - want).max()
    assert np.isnan(C.ls_curvature(np.float32("nan"))[0])


@pytest.mark.parametrize("P,A", [(65, 36), (8616, 36), (16384, 64)])
def test_exact_operands_sum_in_any_order(P, A):
    o = operands(P, A, "exact")
    ref = reference(o, "tail")
    np.testing.assert_array_equal(ref["h"], o["h"])
    rs = np.random.RandomState(0)
    for a, b, want in ((o["p"], ref["z"], ref["pz"]), (ref["r"], ref["r"], ref["rr"])):
        t = a * b
        perm = rs.permutation(P)
        assert want == t.sum() == t[::-1].cumsum()[-1] == t[perm].cumsum()[-1] == float(np.add.reduce(t[perm][::-1]))
    assert ref["v"] == 0.125
    np.testing.assert_array_equal(ref["x"], o["x"] + o["p"] / 8.0)
    np.testing.assert_array_equal(ref["r"] * 64.0, np.round(ref["r"] * 64.0))
