"""tests/gae_ref.py (the comparator of test_gpu_gae_edges.py) pinned without a GPU: to numbers
worked by hand, to oracle.milo_ref, to the reference's own recorded outputs (G9), its grid
decomposition to milo_ref.lanes_to_paths, and numpy's float64 whitening measured against its
higher-precision whitening on every input the GPU test uses (the device's allowance)."""
import numpy as np
import pytest

import gae_cases as C
import gae_ref as G
from oracle import milo_ref as R

f32 = np.float32


# ---- hand-worked -------------------------------------------------------------------------------
def test_hand_worked_terminated_and_cut():
    """r = [1, 2, 3], v = [0.5, 0.25, 0.125], gamma = 0.5, lambda = 0.5 (everything exact).
    returns: 3; 2 + 1.5 = 3.5; 1 + 1.75 = 2.75.
    terminated (b1 = [.5, .25, .125, 0]): delta = [1 + .125 - .5, 2 + .0625 - .25, 3 + 0 - .125]
      = [0.625, 1.8125, 2.875]; adv (gl = .25) = 2.875; 1.8125 + .71875 = 2.53125;
      0.625 + .6328125 = 1.2578125.
    cut (b1 = [.5, .25, .125, .125]): the last delta is 3 + .0625 - .125 = 2.9375; adv = 2.9375;
      1.8125 + .734375 = 2.546875; 0.625 + .63671875 = 1.26171875."""
    r, v = np.array([1, 2, 3], f32), np.array([0.5, 0.25, 0.125], f32)
    ret = G.returns(r, 0.5)
    assert ret.dtype == np.float64
    np.testing.assert_array_equal(ret, [2.75, 3.5, 3.0])
    dt, dc = G.deltas(r, v, True, 0.5), G.deltas(r, v, False, 0.5)
    assert dt.dtype == np.float64 and dc.dtype == np.float32
    np.testing.assert_array_equal(dt, [0.625, 1.8125, 2.875])
    np.testing.assert_array_equal(dc, [0.625, 1.8125, 2.9375])
    at, ac = G.advantages(r, v, True, 0.5, 0.5), G.advantages(r, v, False, 0.5, 0.5)
    assert at.dtype == ac.dtype == np.float64
    np.testing.assert_array_equal(at, [1.2578125, 2.53125, 2.875])
    np.testing.assert_array_equal(ac, [1.26171875, 2.546875, 2.9375])


def test_hand_worked_delta_precision():
    """Where the two delta paths part: r = 1, v = [2^-24] alone in its trajectory, gamma = 1.
    Terminated: 1 + 0 - 2^-24 in float64 = 1 - 2^-24.  Cut: float32(1 + 2^-24) = 1 (tie to even),
    then 1 - 2^-24 is a float32 (the spacing below 1 is 2^-24): the same.  With v = [3 * 2^-25]:
    terminated 1 - 3 * 2^-25; cut float32(1 + 3 * 2^-25) = 1 + 2^-23, minus 3 * 2^-25 = 1 + 2^-25
    -> float32 1 (tie to even) -- the float32 path shows."""
    r = np.array([1], f32)
    for v0, term, cut in [(2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24), (3 * 2.0 ** -25, 1 - 3 * 2.0 ** -25, 1.0)]:
        v = np.array([v0], f32)
        assert G.advantages(r, v, True, 1.0, 1.0)[0] == term
        assert G.advantages(r, v, False, 1.0, 1.0)[0] == cut


@pytest.mark.parametrize("lam", [None, 1.5, -0.1])
def test_hand_worked_standard_mode(lam):
    """returns - baseline, whatever the termination: [2.75 - .5, 3.5 - .25, 3 - .125]."""
    r, v = np.array([1, 2, 3], f32), np.array([0.5, 0.25, 0.125], f32)
    for term in (True, False):
        a = G.advantages(r, v, term, 0.5, lam)
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, [2.25, 3.25, 2.875])
    assert G.standard_mode(lam) and not G.standard_mode(0.0) and not G.standard_mode(1.0)


def test_hand_worked_lane_with_two_trajectories():
    """One lane of 5 rows at rows 10, 13, 16, 19, 22 (base 10, stride 3), end 1 at its third row,
    t0 = 5: trajectory A = rows 10, 13, 16 terminated from position 5, B = rows 19, 22 cut from 0.
    Time features of A's first row (position 5): .005, .000025, 1.25e-7, 6.25e-10; of B's second
    (position 1): .001, 1e-6, 1e-9, 1e-12."""
    end = np.zeros(23, np.uint8)
    end[16] = 1
    trs = G.split(5, 1, [5], [10], 3, end, [5])
    assert [(list(r), t, p) for r, t, p in trs] == [([10, 13, 16], True, 5), ([19, 22], False, 0)]
    obs = np.array([[10.5, -0.0], [-20.0, 5.0], [np.nan, 10.0]])
    fa = G.features(obs, 2, 32, 5 + np.arange(3))
    assert fa.dtype == np.float32 and fa.shape == (3, 32)
    np.testing.assert_array_equal(fa[:, :2], np.array([[1.0, -0.0], [-1.0, 0.5], [np.nan, 1.0]], f32))
    assert np.signbit(fa[0, 1])
    np.testing.assert_array_equal(fa[0, 2:6], np.array([0.005, 0.005 ** 2, 0.005 ** 3, 0.005 ** 4]).astype(f32))
    np.testing.assert_array_equal(fa[0, 2:6], np.array([0.005, 0.000025, 1.25e-7, 6.25e-10], f32))
    assert not fa[:, 6:].any()
    fb = G.features(obs[:2], 2, 32, 0 + np.arange(2))
    np.testing.assert_array_equal(fb[1, 2:6], np.array([1e-3, 1e-6, 1e-9, 1e-12], f32))
    np.testing.assert_array_equal(fb[0, 2:6], np.zeros(4, f32))


def test_hand_worked_head_and_whiten():
    """head: 3 * 0.5 + (-2) * 0.25 + 2^-30 * 1 = 1 + 2^-30 -> float32 1, + 0.5 = 1.5; mag = 2 + 2^-30.
    whiten [1, 2, 3, 6]: mean 3, squared deviations 4 + 1 + 0 + 9 = 14, sd = sqrt(3.5)."""
    v, s, mag = G.head(np.array([3, -2, 2.0 ** -30], f32), np.array([0.5, 0.25, 1], f32), f32(0.5))
    assert v == f32(1.5) and v.dtype == np.float32 and s == 1 + 2.0 ** -30 and mag == 2 + 2.0 ** -30
    out, mean, sd = G.whiten(np.array([1.0, 2.0, 3.0, 6.0]), 0.0)
    assert mean == 3.0 and sd == np.sqrt(3.5)
    np.testing.assert_allclose(out, np.array([-2, -1, 0, 3]) / np.sqrt(3.5), rtol=2e-16)
    assert G.whiten(np.zeros(0), 1e-6)[1:] == (0.0, 0.0)
    out, mean, sd = G.whiten(np.full(7, 0.75), 1e-6)
    assert mean == 0.75 and sd == 0.0 and not out.any()


# ---- oracle and golden -------------------------------------------------------------------------
def random_paths(seed, n_paths=7, S=5):
    rs = np.random.RandomState(seed)
    paths = []
    for i in range(n_paths):
        l = int(rs.randint(1, 40))
        paths.append(dict(observations=rs.randn(l, S) * 6.0, rewards=(rs.randn(l) * 0.3).astype(f32),
                          terminated=bool(i % 2), t0=int(rs.randint(0, 3000)) if i % 3 == 0 else 0,
                          v=rs.randn(l).astype(f32)))
    return paths


def assert_whitened_close(x, got, ref_out, eps):
    """A float64 whitening in any summation order against gae_ref.whiten, at the worst-case bound of
    recursive summation (n 2^-53 of the summed magnitudes, for the mean and for the squared
    deviations): 2 (n + 8) 2^-53 (|x| + mean|x|) / (sd + eps) per element.  (What numpy really
    loses is measured in test_whitening_yardstick.)"""
    _, _, sd = G.whiten(x, eps)
    assert (np.abs(got - ref_out) <= 2 * (x.size + 8) * C.U * (np.abs(x) + np.abs(x).mean()) / (sd + eps)).all()


@pytest.mark.parametrize("gamma,lam", C.GAMMA_LAMBDA)
def test_equals_oracle_on_random_paths(gamma, lam):
    paths = random_paths(3)
    feat = R.mlp_baseline_features(paths)
    R.compute_returns(paths, gamma)
    R.compute_advantages(paths, lambda p: p["v"], gamma, lam)
    k = 0
    for p in paths:
        l = len(p["rewards"])
        np.testing.assert_array_equal(G.features(p["observations"], 5, 32, p["t0"] + np.arange(l))[:, :9], feat[k:k + l])
        np.testing.assert_array_equal(G.returns(p["rewards"], gamma), p["returns"])
        np.testing.assert_array_equal(G.advantages(p["rewards"], p["v"], p["terminated"], gamma, lam), p["advantages"])
        k += l
    adv_w, _ = R.whiten_advantages(paths, eps=1e-6)
    adv = np.concatenate([p["advantages"] for p in paths])
    out, mean, sd = G.whiten(adv, 1e-6)
    assert_whitened_close(adv, adv_w, out, 1e-6)


def test_equals_golden_g9(golden):
    """The reference's own recorded outputs: features, returns and (given the recorded baseline
    values) advantages bit for bit; the whitened advantages (numpy's float64) within the summation bound."""
    g = golden("g9_gae.npz")
    gamma, lam, S = float(g["gamma"]), float(g["gae_lambda"]), g["observations"].shape[1]
    offs = np.concatenate([[0], np.cumsum(g["lengths"])])
    for i, term in enumerate(g["terminated"]):
        sl = slice(offs[i], offs[i + 1])
        f = G.features(g["observations"][sl], S, 256, np.arange(offs[i + 1] - offs[i]))
        np.testing.assert_array_equal(f[:, :8], g["features_head"][sl])
        np.testing.assert_array_equal(f[:, S:S + 4], g["features_time"][sl])
        assert not f[:, S + 4:].any()
        r = g["rewards"][sl]
        np.testing.assert_array_equal(G.returns(r, gamma), g["returns_gae"][sl])
        np.testing.assert_array_equal(G.returns(r, gamma), g["returns_std"][sl])
        np.testing.assert_array_equal(G.advantages(r, g["baseline_gae"][sl], bool(term), gamma, lam), g["adv_gae"][sl])
        np.testing.assert_array_equal(G.advantages(r, g["baseline_std"][sl], bool(term), gamma, None), g["adv_std"][sl])
    x = g["adv_gae"]
    out, mean, sd = G.whiten(x, 1e-6)
    assert_whitened_close(x, g["adv_whitened"], out, 1e-6)


# ---- split -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,seed", [(1, 3, 0), (6, 5, 1), (9, 2, 2)])
def test_split_equals_lanes_to_paths(T, B, seed):
    rs = np.random.RandomState(seed)
    done = (rs.rand(T, B) < 0.3).astype(np.uint8)
    steps0 = rs.randint(0, 50, size=B)
    paths, rows = R.lanes_to_paths(done, np.zeros((T, B), f32), np.zeros((T, B, 1)), steps0)
    trs = G.split(T, B, None, None, B, done.reshape(-1), steps0)
    assert len(trs) == len(paths)
    for (r, term, pos), p, (ts, b) in zip(trs, paths, rows):
        np.testing.assert_array_equal(r, ts * B + b)
        assert term == p["terminated"] and pos == p["t0"]


def test_split_hand_made_grids():
    """len = 0 lanes give nothing; base / stride address the rows; end 2 mid-lane and 0 / 2 at a
    last row are cut, 1 is terminated; t0 only reaches a lane's first trajectory."""
    end = np.zeros(40, np.uint8)
    end[[21, 22, 31]] = [2, 1, 2]
    trs = G.split(4, 4, [0, 3, 4, 2], [0, 20, 30, 7], 1, end, [9, 8, 7, 6])
    got = [(list(r), t, p) for r, t, p in trs]
    assert got == [([20, 21], False, 8), ([22], True, 0), ([30, 31], False, 7), ([32, 33], False, 0),
                   ([7, 8], False, 6)]
    assert G.split(0, 3, None, None, 3, end, None) == [] and G.split(3, 0, None, None, 1, end, None) == []
    got = [(list(r), t, p) for r, t, p in G.split(2, 2, None, None, 2, np.array([1, 0, 0, 2], np.uint8), None)]
    assert got == [([0], True, 0), ([2], False, 0), ([1, 3], False, 0)]


# ---- the GAE cases cannot go blind -------------------------------------------------------------
def test_gae_values_separate_the_delta_paths():
    """On the GPU test's own rewards / values (gae_cases.gae_values, seed 0, the random end flags of
    the 7 x 257 grid): computing a trajectory's deltas in the other precision, or with a fused
    multiply-add, changes at least one advantage of a terminated and of a cut trajectory."""
    T, L = 7, 257
    end = C.end_flags("random", T, L, None, None, L, T * L)
    rew, v = C.gae_values(T * L, 0)
    changed = {(k, t): 0 for k in ("swap", "fma") for t in (True, False)}
    for rows, term, _ in G.split(T, L, None, None, L, end, None):
        d = G.deltas(rew[rows], v[rows], term, 0.995).astype(np.float64)
        for k in ("swap", "fma"):
            changed[(k, term)] += int((G.deltas_mutant(rew[rows], v[rows], term, 0.995, k) != d).sum())
        np.testing.assert_array_equal(G.deltas_mutant(rew[rows], v[rows], term, 0.995, "none"), d)
    print("advantage deltas changed by the substitution:", changed)
    assert all(n > 0 for n in changed.values()), changed


# ---- the whitening yardstick -------------------------------------------------------------------
def test_whitening_yardstick():
    """numpy's float64 (x - x.mean()) / (x.std() + eps) against gae_ref.whiten on every whitening
    input of test_gpu_gae_edges.py, per element in units of 2^-53 (|x| + |mean|) / (sd + eps), the
    mean in 2^-53 |mean|, sd in 2^-53 sd.  Measured maxima (numpy 2.2, x86-64): elem 3.04
    (flat1023), mean 1.66 (emptychunk), sd 3.86 (ill1e6: numpy's own float64 mean is 0.25 ulp from
    the true one there); in most cases numpy's mean and sd are the correctly rounded ones.  Recorded
    rounded up as gae_cases.NUMPY_MAX = 3.1 / 1.7 / 3.9, and the device is allowed gae_cases.MARGIN = 4 / 4 / 16
    times that (the reasoning stands there).  This test prints the maxima and fails if numpy ever
    measures above what is recorded, so the allowance cannot be wider than the measurement says."""
    worst = {"elem": (0.0, ""), "mean": (0.0, ""), "sd": (0.0, "")}
    for c in C.whiten_cases():
        x = c["buf"][c["rows"]]
        assert not np.isnan(x).any()
        ref = G.whiten(x, C.EPS)
        if x.size == 0:
            assert ref[1:] == (0.0, 0.0)
            continue
        with np.errstate(all="ignore"):
            e = C.whiten_errors(x, (x - x.mean()) / (x.std() + C.EPS), x.mean(), x.std(), *ref, C.EPS)
        print(f"WHITEN numpy {c['name']}: elem {e[0]:.2f} mean {e[1]:.2f} sd {e[2]:.2f}")
        for k, v in zip(worst, e):
            if v > worst[k][0]:
                worst[k] = (v, c["name"])
    print("WHITEN numpy maxima:", worst)
    for k in worst:
        assert worst[k][0] <= C.NUMPY_MAX[k], (k, worst[k])
        assert worst[k][0] > 0.5 * C.NUMPY_MAX[k], ("the recorded maximum is stale", k, worst[k])


def test_whitening_cases_are_what_they_claim():
    """The empty-chunk case leaves whole 4096-cell chunks without a valid cell (from the index
    arithmetic t = i // L, l = i % L), the ragged case has cells in more than one chunk, the
    ill-conditioned inputs defeat a sum-of-squares formula by orders of magnitude."""
    cases = {c["name"]: c for c in C.whiten_cases()}
    c = cases["emptychunk"]
    total = c["T"] * c["L"]
    valid = [i for i in range(total) if i // c["L"] < c["len"][i % c["L"]]]
    assert sorted(valid) == sorted(c["cells"].tolist())
    chunks = {i // 4096 for i in valid}
    assert (total + 4095) // 4096 == 4 and chunks == {0}, chunks
    c = cases["leadempty"]
    assert {int(i) // 4096 for i in c["cells"]} == {1, 2}
    c = cases["ragged1300x7"]
    assert {int(i) // 4096 for i in c["cells"]} == {0, 1, 2} and set(c["len"][[0, 1, 2]]) == {0, 1, 1300}
    for name in ("ill1e6", "ill-3e8"):
        x = cases[name]["buf"][cases[name]["rows"]]
        _, mean, sd = G.whiten(x, C.EPS)
        one_pass = np.sqrt(abs((x * x).sum() / x.size - x.mean() ** 2))
        assert abs(one_pass - sd) / (C.U * sd) > 1e4 * C.ALLOW["sd"], (name, one_pass, sd)
