"""numpy fp64 restatement of the DTW evaluation score (the comparator of test_cpu_dtw.py and
test_gpu_dtw.py): DeepMimicCore's cDynamicTimeWarper, the time-warp rows it is fed, and the
score cSceneImitateAMP reports.  Paths are relative to deepmimic/deepmimic/DeepMimicCore/.

Written from the behaviour of the cited lines; operation order follows them where the result
depends on it (the `<=` rules of the backtrack, the running cost, division before the
multiplication in the remainder).  Where the C++ leaves the association of a sum to Eigen's
vectorisation (`norm()` of a point difference, `sum()` of the backtrack) the sums here run in
index order; on exactly summable data every order gives the same bits.

The scene builds its warper with TimeWarpCost (scenes/SceneImitateAMP.cpp:510), so that is the
cost of the reported `dtw_cost` and the default here; DefaultCost is what a warper initialised
without a cost function uses (util/DynamicTimeWarper.cpp:30-37)."""
import math

import numpy as np

from oracle import deepmimic_ref as D


# ---- the two cell costs ------------------------------------------------------------------------
def time_warp_cost(data0, data1):
    """cSceneImitateAMP::TimeWarpCost (scenes/SceneImitateAMP.cpp:5-25) for every pair of rows:
    the rows as dim / 3 points (:12-17), per point the Euclidean distance of pt1 - pt0 (:18; the
    4-vector's w is 0), added up in point order (:19) and divided by the number of points (:22)."""
    n, m, dim = len(data0), len(data1), data0.shape[1]
    assert dim % 3 == 0 and data1.shape[1] == dim
    val = np.zeros((n, m))
    for p in range(dim // 3):
        d = data1[None, :, 3 * p:3 * p + 3] - data0[:, None, 3 * p:3 * p + 3]
        val = val + np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    return val / (dim // 3)


def default_cost(data0, data1):
    """cDynamicTimeWarper::DefaultCost (util/DynamicTimeWarper.cpp:3-8) for every pair of rows:
    the squared norm of the difference."""
    diff = data0[:, None, :] - data1[None, :, :]
    return (diff * diff).sum(axis=2)


COSTS = {"points": time_warp_cost, "squared": default_cost}


# ---- util/DynamicTimeWarper.cpp -------------------------------------------------------------
def cost_buffer(data0, data1, cost="points"):
    """CalcAlignment (util/DynamicTimeWarper.cpp:119-146): the n x m cost buffer.  C(0,0) = 0,
    the rest of row 0 and column 0 +inf (:123-124); cells i, j >= 1 are the cell cost (CalcCost,
    :133, 251-255: the function Init was given) plus the least of the three predecessors
    (:134-141).  Sample 0 of either side is never scored (both loops start at 1, :126, 129)."""
    data0, data1 = np.asarray(data0, np.float64), np.asarray(data1, np.float64)
    n, m = len(data0), len(data1)
    C = np.full((n, m), np.inf)
    C[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        val = COSTS[cost](data0, data1)
    for i in range(1, n):
        for j in range(1, m):
            C[i, j] = val[i, j] + min(C[i - 1, j - 1], min(C[i - 1, j], C[i, j - 1]))
    return C


def backtrack(C):
    """CalcIndexBuffer (util/DynamicTimeWarper.cpp:148-200) on a cost buffer: (index [n] int,
    backtrack [n]).  From (n-1, m-1) while i >= 1 and j >= 1 (:158): index[i] = j on every visit
    (:160); diagonal when cost0 <= cost1 and cost0 <= cost2 (:167), else up when cost1 <= cost2
    (:176), else left (:184); a left move only accumulates the running cost (:186), the other two
    write backtrack[i] and clear it (:169-171, 178-180); i, j clamped at 0 (:189-190).  Rows
    [0, i] then get index 0 (:192) and backtrack = the self-cost of a sample, 0 (:195-198)."""
    n, m = C.shape
    index = np.zeros(n, np.int32)
    bt = np.zeros(n)
    i, j = n - 1, m - 1
    run = 0.0
    while i >= 1 and j >= 1:
        index[i] = j
        total, c0, c1, c2 = C[i, j], C[i - 1, j - 1], C[i - 1, j], C[i, j - 1]
        if c0 <= c1 and c0 <= c2:
            run += total - c0
            bt[i] = run
            run = 0.0
            i, j = i - 1, j - 1
        elif c1 <= c2:
            run += total - c1
            bt[i] = run
            run = 0.0
            i -= 1
        else:
            run += total - c2
            j -= 1
        i, j = max(0, i), max(0, j)
    index[:i + 1] = 0
    bt[:i + 1] = 0.0
    return index, bt


def add_remainder(bt, remainder):
    """AddRemainderCost (util/DynamicTimeWarper.cpp:202-214): backtrack += (backtrack /
    sum(backtrack)) * remainder over the first n entries (:212-213); the sum runs in index
    order here.  An all-zero backtrack gives NaN, as there."""
    bt = np.asarray(bt, np.float64)
    s = 0.0
    for v in bt:
        s += v
    with np.errstate(invalid="ignore", divide="ignore"):
        return bt + (bt / s) * remainder


def align(data0, data1, buffer_size=None, cost="points"):
    """The warper's whole answer for one pair of row sequences of equal length n:
    cost = C(n-1, m-1) (GetMinAlignmentCost, :243-249), remainder = (buffer_size - n) * 1.0
    (scenes/SceneImitateAMP.cpp:263-266), dtw_cost = cost + remainder (:266-269)."""
    C = cost_buffer(data0, data1, cost)
    n = len(C)
    index, raw = backtrack(C)
    remainder = float((n if buffer_size is None else buffer_size) - n) * 1.0
    return dict(C=C, cost=C[-1, -1], index=index, backtrack_raw=raw, backtrack=add_remainder(raw, remainder),
                remainder=remainder, dtw_cost=C[-1, -1] + remainder)


def min_predecessor_gap(C):
    """The smallest gap between the two best predecessors over the cells i, j >= 2 (where all
    three are finite): how far a rounding difference is from changing a backtrack decision."""
    a = np.stack([C[1:-1, 1:-1], C[1:-1, 2:], C[2:, 1:-1]])
    a.sort(axis=0)
    return float((a[1] - a[0]).min())


# ---- scenes/SceneImitateAMP.cpp:537-555 (BuildTimeWarpData) ----------------------------------
def rows_from_pose(joints, pose, root_y=None):
    """[(0, root_y, 0), joint_j - root joint (world) for j >= 1] of a pose (:542-554), the joint
    origins from the oracle's forward kinematics."""
    _, o, _, _ = D.forward_kinematics(joints, pose, np.zeros(len(pose)))
    row = np.zeros(3 * len(joints))
    row[1] = pose[1] if root_y is None else root_y
    for j in range(1, len(joints)):
        row[3 * j:3 * j + 3] = o[j] - o[0]
    return row


def rows_from_state(joints, bodies, s):
    """The same row from a recorded state (CtController layout, RecordWorldRootRot only): the
    state holds pp_j = Rh (body_j - root joint) and the body rotations in the heading frame as
    tangent-normal pairs, body_j = joint_j + R_j attach_body_j, so joint_j - root joint =
    Rh^T (pp_j - R^h_j attach_body_j); root_y = s[0]."""
    s = np.asarray(s, np.float64)
    Rw0 = D._tn_mat(s[4:10])
    Rh = D.rotmat_axis((0.0, 1.0, 0.0), -math.atan2(-Rw0[2, 0], Rw0[0, 0]))
    row = np.zeros(3 * len(joints))
    row[1] = s[0]
    for j in range(1, len(joints)):
        Rj = D._tn_mat(s[9 * j + 4:9 * j + 10])
        row[3 * j:3 * j + 3] = Rh.T @ (s[9 * j + 1:9 * j + 4] - Rj @ bodies[j]["attach"])
    return row


def rows_from_motion(joints, M, t0, n, lift=0.0, update_rate=30.0):
    """Rows of the kinematic character for a trajectory reset at clip time t0: row i is the pose
    at t0 + i / update_rate (the warper is sampled once per control step, :194-204, 523-535), the
    root height raised by the trajectory's ground-resolve lift (SyncKinCharRoot,
    scenes/SceneImitate.cpp:550-582) until a looping clip starts its next cycle: UpdateKinChar
    (:400-412) then calls SyncKinCharNewCycle, which sets the root height to the ground's plus
    the clip's height over the origin (:601-606), and the lift is gone from there on."""
    out = np.zeros((n, 3 * len(joints)))
    for i in range(n):
        t = t0 + i / update_rate
        pose = M.pose(t)
        lifted = not M.loop or math.floor(t / M.duration) == math.floor(t0 / M.duration)
        out[i] = rows_from_pose(joints, pose, pose[1] + lift if lifted else pose[1])
    return out


def reset_lift(joints, bodies, M, t0, resolve=True):
    """s_0[0] - clip_root_y(t0): how far the ground resolve raised the character at reset."""
    if not resolve:
        return 0.0
    return D.reset_state(joints, bodies, M, t0)[0] - M.pose(t0)[1]


# ---- scenes/SceneImitateAMP.cpp:243-272 (CalcRewardTimeWarp) ---------------------------------
def buffer_size(update_rate=30.0, time_end_max=10.0):
    """BuildTimeWarper (:503-507): ceil(update_rate * max time) + 2."""
    return int(math.ceil(update_rate * time_end_max)) + 2


def score(joints, bodies, M, states, t0, update_rate=30.0, time_end_max=10.0, resolve=True):
    """dtw_cost of one trajectory from its T + 1 recorded states and its reset time, with the
    scene's cell cost (TimeWarpCost)."""
    states = np.asarray(states, np.float64)
    n = len(states)
    sim = np.stack([rows_from_state(joints, bodies, s) for s in states])
    lift = states[0, 0] - M.pose(t0)[1] if resolve else 0.0
    kin = rows_from_motion(joints, M, t0, n, lift, update_rate)
    return align(sim, kin, buffer_size(update_rate, time_end_max), "points")
