"""The DTW evaluation score on the device (csrc/amx_dtw.hip, the time-warp rows of
csrc/amx_motion.hip, dtw.TimeWarper, sample_points(dtw=...), evaluate) vs the numpy fp64
restatement tests/dtw_ref.py of DeepMimicCore's cDynamicTimeWarper and BuildTimeWarpData.

The kernel has the warper's two cell costs: TimeWarpCost ('points': the mean Euclidean distance
of the rows' 15 points, what the scene's warper is built with and `dtw_cost` means) and
DefaultCost ('squared').  Bounds: on a dyadic grid every square and partial sum is exact in fp64
(for 'points': on rows whose point differences have one nonzero component or are multiples of a
Pythagorean triple, so every square root is exact too), so the alignment is compared bit for
bit; on generic data only the summation order of a squared distance (45 terms) or the last bit
of a square root differs, a few ulp, so index paths are equal wherever predecessors are 1e-9
apart and costs agree to 1e-12 relative per element; the rows differ by device vs host libm last
bits on O(1) values: 1e-12 absolute.  Parity with the C++ core itself is unpinned (it cannot be built)."""
import json
import types

import numpy as np
import pytest
import torch

import dtw_ref as R
from oracle import deepmimic_ref as D
from oracle import milo_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, A = 226, 28
TI, TJ = 32, 64  # the kernel's val tile: rows of data0 x rows of data1 (csrc/amx_dtw.hip)


@pytest.fixture(scope="module")
def setup(golden):
    import amp_extensions_amd as amx
    from amp_extensions_amd.ensemble import init_ensemble_weights
    from amp_extensions_amd.motion import ReferenceMotion
    g = golden("g12_motion.npz")
    char = json.loads(str(g["character_json"]))
    motion = {"Loop": str(g["loop"]), "Frames": g["frames"].tolist()}
    rs = np.random.RandomState(0)
    s = 0.5 * rs.randn(2048, S)
    a = rs.randn(2048, A)
    s2 = s + 0.01 * rs.randn(2048, S)
    norms = MR.get_transformations(*[torch.from_numpy(x).float() for x in (s, a, s2)])
    ctx = amx.AmxContext(S, A, n_models=4, hidden=64, n_hidden=4, feat_dim=512, device=DEV)
    ens = amx.DeviceEnsemble(ctx, init_ensemble_weights(S, A, [64] * 4, 4, 100), norms)
    rm = ReferenceMotion(ctx, char, motion)
    J, B, _ = D.load_character(char)
    M = D.Motion(motion, J)
    tw = amx.TimeWarper(ctx, rm)
    assert tw.buffer_size == R.buffer_size() == 302 and tw.dim == 3 * len(J) == 45
    return types.SimpleNamespace(amx=amx, ctx=ctx, ens=ens, rm=rm, J=J, B=B, M=M, tw=tw)


def raw_align(ctx, d0, d1, lens, buffer_size, kind="squared"):
    """amx_dtw_align with canary-filled outputs: numpy (cost, dtw_cost, index, raw, backtrack)."""
    from amp_extensions_amd import _native as N
    T, n_max, dim = d0.shape
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    a, b = dev(d0), dev(d1)
    ln = np.ascontiguousarray(lens, np.int32)
    ln_dev = dev(ln)
    work = torch.empty(int(ctx.lib.amx_dtw_work(T, n_max)), dtype=torch.float64, device=DEV)
    cost = torch.full((T,), -1.0, dtype=torch.float64, device=DEV)
    dtw = torch.full((T,), -1.0, dtype=torch.float64, device=DEV)
    index = torch.full((T, n_max), -7, dtype=torch.int32, device=DEV)
    raw = torch.full((T, n_max), 12345.0, dtype=torch.float64, device=DEV)
    bt = torch.full((T, n_max), 12345.0, dtype=torch.float64, device=DEV)
    kind = {"squared": N.AMX_DTW_COST_SQUARED, "points": N.AMX_DTW_COST_POINTS}[kind]
    N.check(ctx.lib.amx_dtw_align(ctx.h, a.data_ptr(), b.data_ptr(), dim, dim, kind, n_max, ln.ctypes.data,
                                  ln_dev.data_ptr(), T, buffer_size, work.data_ptr(), cost.data_ptr(), dtw.data_ptr(),
                                  index.data_ptr(), raw.data_ptr(), bt.data_ptr(), ctx.stream), "amx_dtw_align")
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (cost, dtw, index, raw, bt))


def check_exact(ctx, d0, d1, lens, buffer_size, kind="squared"):
    cost, dtw, index, raw, bt = raw_align(ctx, d0, d1, lens, buffer_size, kind)
    ties = 0
    for t, n in enumerate(lens):
        r = R.align(d0[t, :n], d1[t, :n], buffer_size, kind)
        assert cost[t] == r["cost"] and dtw[t] == r["dtw_cost"], (t, n, cost[t], r["cost"])
        np.testing.assert_array_equal(index[t, :n], r["index"], err_msg=f"index, trajectory {t} (len {n})")
        np.testing.assert_array_equal(raw[t, :n], r["backtrack_raw"], err_msg=f"backtrack, trajectory {t} (len {n})")
        np.testing.assert_array_equal(bt[t, :n], r["backtrack"], err_msg=f"backtrack + remainder, trajectory {t}")
        # nothing past the trajectory's length is written
        assert (index[t, n:] == -7).all() and (raw[t, n:] == 12345.0).all() and (bt[t, n:] == 12345.0).all()
        if n >= 4:
            ties += int(R.min_predecessor_gap(r["C"]) == 0.0)
    return ties


def test_alignment_exact_on_dyadic_grid(setup):
    """The warper's DefaultCost (squared distances).  Integer multiples of 2^-6 in [-2, 2]: cost,
    index, backtrack before and after the remainder equal the restatement bit for bit, at every length class in ONE launch (the shortest, odd,
    around the edges of the 32 x 64 val tile (rows 1 .. n-1 are tiled), several tiles, the full 302
    buffer; the sweep has no passes: one thread per row), rows past each length NaN; then a
    coarse low-dimensional grid, where ties between predecessors abound and the `<=` rules decide;
    then identical sequences (a free diagonal; the remainder of an all-zero backtrack is NaN on
    both sides)."""
    ctx = setup.ctx
    rs = np.random.RandomState(5)
    lens = [2, 3, 17, TI + 1, TI + 2, 64, TJ + 1, TJ + 2, 257, 258, 301, 302]
    n_max, dim = 302, 45
    d0 = rs.randint(-128, 129, (len(lens), n_max, dim)) / 64.0
    d1 = rs.randint(-128, 129, (len(lens), n_max, dim)) / 64.0
    for t, n in enumerate(lens):
        d0[t, n:] = np.nan
        d1[t, n:] = np.nan
    check_exact(ctx, d0, d1, lens, 302)
    # coarse grid, dim 3: multiples of 1/2 in [-1, 1]
    lens = [17, 66, 258]
    d0 = rs.randint(-2, 3, (3, 258, 3)) / 2.0
    d1 = rs.randint(-2, 3, (3, 258, 3)) / 2.0
    for t, n in enumerate(lens):
        d0[t, n:] = np.nan
        d1[t, n:] = np.nan
    assert check_exact(ctx, d0, d1, lens, 400) == 3   # every trajectory has tied predecessors
    # identical sequences
    d = rs.randint(-128, 129, (2, 70, 45)) / 64.0
    cost, dtw, index, raw, bt = raw_align(ctx, d, d, [70, 33], 302)
    check_exact(ctx, d, d, [70, 33], 302)
    assert (cost == 0.0).all() and (index[0] == np.arange(70)).all() and np.isnan(bt[0]).all()


def test_alignment_exact_time_warp_cost(setup):
    """TimeWarpCost on rows whose every point distance is exact: even points differ in one
    component (multiples of 2^-6 on both sides: sqrt(x^2) = |x|), odd points are 0 on one side
    and a multiple of a Pythagorean triple / 64 on the other ((3,4,0) -> 5, (0,5,12) -> 13,
    (8,0,15) -> 17, (2,3,6) -> 7).  The 15 distances are multiples of 2^-6, their sum is exact in
    any order and the division by 15 rounds once: bit for bit, ties included."""
    ctx = setup.ctx
    rs = np.random.RandomState(6)
    lens = [2, 3, TI + 2, TJ + 2, 258, 302]
    T, n_max, J = len(lens), 302, 15
    triples = np.array([[3, 4, 0], [0, 5, 12], [8, 0, 15], [2, 3, 6]], np.float64)
    d0 = np.zeros((T, n_max, J, 3))
    d1 = np.zeros((T, n_max, J, 3))
    for p in range(J):
        if p % 2 == 0:
            d0[:, :, p, p % 3] = rs.randint(-128, 129, (T, n_max)) / 64.0
            d1[:, :, p, p % 3] = rs.randint(-128, 129, (T, n_max)) / 64.0
        else:
            d1[:, :, p] = rs.randint(-4, 5, (T, n_max, 1)) * triples[rs.randint(0, 4, (T, n_max))] / 64.0
    d0, d1 = d0.reshape(T, n_max, 45), d1.reshape(T, n_max, 45)
    for t, n in enumerate(lens):
        d0[t, n:] = np.nan
        d1[t, n:] = np.nan
    check_exact(ctx, d0, d1, lens, 302, "points")
    # a coarse grid (one point, one component, multiples of 1/2): predecessors tie
    lens = [17, 66, 258]
    d0 = np.zeros((3, 258, 3))
    d1 = np.zeros((3, 258, 3))
    d0[:, :, 1] = rs.randint(-2, 3, (3, 258)) / 2.0
    d1[:, :, 1] = rs.randint(-2, 3, (3, 258)) / 2.0
    assert check_exact(ctx, d0, d1, lens, 400, "points") == 3


@pytest.mark.parametrize("kind", ["squared", "points"])
def test_alignment_generic_data(setup, kind):
    """40 kinematic rows of the clip from t0 = 0.3 against themselves + 0.02 N(0, 1): predecessors
    are never closer than 1e-9 on the restatement (2.5e-3 with the squared cost, 1.1e-3 with
    TimeWarpCost), so the index path must be equal; cost and every backtrack entry within 1e-12
    relative, plus the cancellation floor of an entry (a difference of two path costs, each a few
    ulp of the final cost off): 8 eps x the final cost."""
    kin = R.rows_from_motion(setup.J, setup.M, 0.3, 40)
    sim = kin + 0.02 * np.random.RandomState(1).randn(*kin.shape)
    ref = R.align(sim, kin, 302, kind)
    gap = R.min_predecessor_gap(ref["C"])
    print(kind, "smallest gap between the two best predecessors:", gap)
    assert gap >= 1e-9
    got = setup.tw.align(sim, kin, [40], buffer_size=302, cost=kind)
    got = {k: v.cpu().numpy()[0] for k, v in got.items()}
    np.testing.assert_array_equal(got["index"], ref["index"])
    floor = 8 * np.finfo(np.float64).eps * ref["cost"]
    for k in ("cost", "dtw_cost", "backtrack_raw", "backtrack"):
        err = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)
        print(kind, k, "largest relative error of an element", err.max())
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=floor, err_msg=k)
    if kind == "points":   # the warper's own cost is the scene's
        assert setup.tw.cost == "points"
        same = setup.tw.align(sim, kin, [40], buffer_size=302)
        np.testing.assert_array_equal(same["backtrack"].cpu().numpy()[0], got["backtrack"])


def _reorthonormalise(s, nj):
    """Each body's (normal, tangent) pair made orthonormal again (Gram-Schmidt from the normal)."""
    s = s.copy()
    for j in range(nj):
        n, t = s[9 * j + 4:9 * j + 7], s[9 * j + 7:9 * j + 10]
        n = n / np.linalg.norm(n)
        t = t - (t @ n) * n
        s[9 * j + 4:9 * j + 7], s[9 * j + 7:9 * j + 10] = n, t / np.linalg.norm(t)
    return s


def test_state_rows(setup):
    """Rows from recorded states vs the restatement: 64 reset states, and the same states
    perturbed and re-orthonormalised (arbitrary, dynamics-like states)."""
    rs = np.random.RandomState(2)
    reset = setup.rm.states(rs.uniform(0, 2 * setup.M.duration, 64)).cpu().numpy()
    noisy = np.stack([_reorthonormalise(s, len(setup.J)) for s in reset + 0.05 * rs.randn(*reset.shape)])
    for name, states in (("reset", reset), ("perturbed", noisy)):
        got = setup.tw.rows_from_states(torch.from_numpy(states)).cpu().numpy()
        ref = np.stack([R.rows_from_state(setup.J, setup.B, s) for s in states])
        err = np.abs(got - ref).max()
        print(name, "state rows: max abs error", err)
        assert got.shape == (64, 45) and err <= 1e-12, (name, err)
    # a broadcast view (row stride 0) is read as the rows it stands for
    rep = setup.tw.rows_from_states(torch.from_numpy(noisy[:1]).to(DEV).expand(5, S)).cpu().numpy()
    np.testing.assert_array_equal(rep, np.repeat(got[:1], 5, axis=0))
    # other record-flag sets are refused, by the surface and by the library
    c = setup.ctx
    out = torch.zeros(4, 45, dtype=torch.float64, device=DEV)
    st = torch.from_numpy(reset[:4]).to(DEV)
    assert c.lib.amx_state_tw_rows(c.h, st.data_ptr(), S, 4, 3, out.data_ptr(), 45, c.stream) == -1
    assert b"RecordWorldRootRot" in c.lib.amx_last_error()
    assert c.lib.amx_state_tw_rows(c.h, st.data_ptr(), S, 4, 2, out.data_ptr(), 44, c.stream) == -1
    tw = setup.amx.TimeWarper(c, setup.rm)
    tw.motion = types.SimpleNamespace(flags=3)   # a motion recorded with RecordWorldRootPos as well
    with pytest.raises(NotImplementedError):
        tw.rows_from_states(st)


def test_motion_rows(setup):
    """Rows of the kinematic character for 8 start times x 12 steps with nonzero lifts, two of
    them crossing a cycle boundary of the looping clip."""
    M = setup.M
    assert M.loop
    rs = np.random.RandomState(3)
    t0 = np.concatenate([[0.0, M.duration - 0.2, 2 * M.duration - 0.1], rs.uniform(0, M.duration, 5)])
    lift = rs.uniform(0.01, 0.1, 8)
    got = setup.tw.rows_from_motion(t0, 12, lift).cpu().numpy()
    ref = np.stack([R.rows_from_motion(setup.J, M, float(t), 12, float(l)) for t, l in zip(t0, lift)])
    err = np.abs(got - ref).max()
    print("motion rows: max abs error", err)
    assert got.shape == (8, 12, 45) and err <= 1e-12
    # the lift holds for the rows of the cycle a trajectory was reset in and is gone after it
    # (SyncKinCharNewCycle): trajectory 1 (reset 0.2 s before the clip's end) is in the next cycle from row 6 on
    bare = setup.tw.rows_from_motion(t0, 12).cpu().numpy()
    cyc = np.floor((t0[:, None] + np.arange(12) / 30.0) / M.duration) == np.floor(t0 / M.duration)[:, None]
    assert cyc[1, :6].all() and not cyc[1, 6:].any() and cyc[2, :3].all() and not cyc[2, 3:].any()
    np.testing.assert_array_equal(got[:, :, 1], np.where(cyc, bare[:, :, 1] + lift[:, None], bare[:, :, 1]))
    one = setup.tw.rows_from_motion(float(t0[1]), 12, float(lift[1])).cpu().numpy()
    np.testing.assert_array_equal(one, got[1])
    # no lift = a lift of zero
    np.testing.assert_array_equal(setup.tw.rows_from_motion(t0, 12).cpu().numpy(),
                                  setup.tw.rows_from_motion(t0, 12, np.zeros(8)).cpu().numpy())


@pytest.fixture(scope="module")
def sampled(setup):
    amx = setup.amx
    pw, log_std = MR.init_policy_weights(S, A, (32, 32), seed=100, init_log_std=-0.25)
    pol = amx.DevicePolicy(setup.ctx, pw, log_std)
    env = amx.BatchedSimEnv(setup.ens, setup.rm, lanes=64, horizon=12, record_means=True)
    kw = dict(num_to_collect=4, base_seed=3, num_workers=2, mode="trajectories")
    return env, pol, kw, amx.sample_points(env, pol, dtw=setup.tw, **kw)


def test_sampler_delivers_dtw_cost(setup, sampled):
    env, pol, kw, paths = sampled
    assert len(paths) == 4
    again = setup.tw.score_paths(paths)
    cost, dtw = again["cost"].cpu().numpy(), again["dtw_cost"].cpu().numpy()
    for k, p in enumerate(paths):
        T = len(p["rewards"])
        delivered = p["env_infos"][-1]["dtw_cost"]
        assert all(x == {} for x in p["env_infos"][:-1]) and set(p["env_infos"][-1]) == {"dtw_cost"}
        assert isinstance(delivered, float) and delivered == dtw[k]          # bit for bit
        states = np.concatenate([p["observations"], p["next_observations"][-1:]], axis=0)
        ref = R.score(setup.J, setup.B, setup.M, states, p["reset_time"])
        print("path", k, "T", T, "dtw_cost", delivered, "restated", ref["dtw_cost"])
        assert abs(delivered - ref["dtw_cost"]) <= 1e-9 * abs(ref["dtw_cost"])
        assert ref["remainder"] == 302 - (T + 1) and dtw[k] == cost[k] + (302 - (T + 1))
        assert len(again["backtrack"][k]) == len(again["index"][k]) == T + 1
        # the reset time is the one the trajectory's reset drew: its first state is the clip's there
        np.testing.assert_array_equal(p["observations"][0], setup.rm.states([p["reset_time"]]).cpu().numpy()[0])
    # without dtw the dicts are today's
    plain = setup.amx.sample_points(env, pol, **kw)
    for p, q in zip(plain, paths):
        assert "reset_time" not in p and all(x == {} for x in p["env_infos"])
        assert set(q) == set(p) | {"reset_time"}
        np.testing.assert_array_equal(p["observations"], q["observations"])
    # the device-drawn reset times reach the paths too
    dev = setup.amx.sample_points(env, pol, dtw=setup.tw, rng="device", **kw)
    for p in dev:
        np.testing.assert_array_equal(p["observations"][0], setup.rm.states([p["reset_time"]]).cpu().numpy()[0])
        assert np.isfinite(p["env_infos"][-1]["dtw_cost"])


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


class _Writer:
    def __init__(self):
        self.scalars, self.groups = {}, {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = (float(value), step)

    def add_scalars(self, tag, values, step):
        self.groups[tag] = ({k: float(v) for k, v in values.items()}, step)


def test_evaluate_delivery(setup, sampled):
    from amp_extensions_amd.evaluate import evaluate
    amx = setup.amx
    env, pol, _, _ = sampled
    rs = np.random.RandomState(7)
    es = setup.rm.states(rs.uniform(0, setup.M.duration, 256)).cpu().numpy()
    expert = torch.from_numpy(np.concatenate([es, es + 0.01 * rs.randn(*es.shape)], axis=1)).float()
    cost = amx.RBFLinearCost(expert, feature_dim=512, input_type="ss", seed=100, ctx=setup.ctx)
    args = types.SimpleNamespace(seed=5, num_cpu=2, cost_input_type="ss")
    log, wr = _Log(), _Writer()
    scores, costs = evaluate(2, log, wr, args, env, pol, cost, num_traj=4)
    assert set(scores) == set(costs) == {"greedy", "sample"}
    greedy = amx.sample_points(env, pol, num_to_collect=4, base_seed=7, num_workers=2, mode="trajectories",
                               eval_mode=True, dtw=setup.tw)
    want = np.mean([p["env_infos"][-1]["dtw_cost"] for p in greedy])
    assert scores["greedy"] == want
    x = torch.from_numpy(np.concatenate([np.concatenate([p["observations"], p["next_observations"]], axis=1)
                                         for p in greedy])).float()
    diff = cost.get_rep(x).mean(0) - cost.phi_e
    mmd, want_mmd = float(costs["greedy"]), float(torch.dot(diff, diff))
    print("greedy MMD", mmd, "recomputed", want_mmd)
    assert want_mmd > 0 and abs(mmd - want_mmd) <= 1e-6 * want_mmd
    assert set(wr.groups) == {"data/inf_greedy_dtw_cost", "data/inf_sampled_dtw_cost"}
    assert set(wr.scalars) == {"data/inf_greedy_len", "data/greedy_mmd", "data/inf_sampled_len", "data/sampled_mmd"}
    g, step = wr.groups["data/inf_greedy_dtw_cost"]
    assert step == 3 and set(g) == {"min_score", "mean_score", "max_score"} and g["mean_score"] == want
    assert wr.scalars["data/greedy_mmd"][0] == mmd
    assert log.lines[0] == "=== Evaluating with seed: 7 ===" and len(log.lines) == 7
    assert log.lines[1].startswith("Greedy Evaluation DTW Cost mean (min, max): ")
    assert log.lines[4].startswith("Sampled Evaluation DTW Cost mean (min, max): ")
    assert log.lines[3].startswith("Greedy MMD: ") and log.lines[6].startswith("Sampled MMD: ")
