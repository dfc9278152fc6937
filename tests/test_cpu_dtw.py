"""CPU-only checks of the DTW evaluation score: the restatement tests/dtw_ref.py is pinned on a
hand-worked case and its two row builders agree on reset states; the new entry points are
declared, bound and exported, and refuse bad arguments before anything touches a GPU."""
import ctypes
import json

import numpy as np
import pytest

import dtw_ref as R
from amp_extensions_amd import _build, _native
from oracle import deepmimic_ref as D

NEW = ("amx_tw_dim", "amx_state_tw_rows", "amx_motion_tw_rows", "amx_dtw_work", "amx_dtw_align")
INF = np.inf


@pytest.fixture(scope="module")
def lib():
    return _native.load(_build.build(verbose=False))


@pytest.fixture(scope="module")
def clip(golden):
    g = golden("g12_motion.npz")
    char = json.loads(str(g["character_json"]))
    J, B, _ = D.load_character(char)
    return J, B, D.Motion({"Loop": str(g["loop"]), "Frames": g["frames"].tolist()}, J)


def test_state_rows_equal_pose_rows_on_reset_states(clip):
    """BuildTimeWarpData read from a recorded reset state equals the same rows read from the pose
    the state was recorded from (root height included: the state's root_y carries the lift)."""
    J, B, M = clip
    worst = 0.0
    for t in np.random.RandomState(0).uniform(0, M.duration, 20):
        s = D.reset_state(J, B, M, float(t))
        pose, _ = D.reset_pose_vel(J, B, M, float(t))
        worst = max(worst, np.abs(R.rows_from_state(J, B, s) - R.rows_from_pose(J, pose)).max())
        # and the kinematic row at the reset time with the reset lift is the same row
        kin = R.rows_from_motion(J, M, float(t), 1, R.reset_lift(J, B, M, float(t)))[0]
        worst = max(worst, np.abs(R.rows_from_state(J, B, s) - kin).max())
    print("state rows vs pose rows:", worst)
    assert worst <= 1e-12


def test_hand_worked_alignment():
    """The warper's routines with its DefaultCost (dim 1 holds no 3-d points).
    data0 = (., 1, 5, 6), data1 = (., 2, 0, 5), dim 1; sample 0 of both is never scored.
    val:  i=1: 1 1 16 | i=2: 9 25 0 | i=3: 16 36 1
    C:    row 1: 1, 1+1=2, 16+2=18 | row 2: 9+1=10, 25+min(1,2,10)=26, 0+min(2,18,26)=2
          row 3: 16+10=26, 36+min(10,26,26)=46, 1+min(26,2,46)=3
    walk: (3,3) preds (26, 2, 46): up, backtrack[3] = 3-2 = 1;  (2,3) preds (2, 18, 26): diagonal,
          backtrack[2] = 2-2 = 0;  (1,2) preds (inf, inf, 1): LEFT, running cost 2-1 = 1;
          (1,1) preds (0, inf, inf): diagonal, backtrack[1] = 1 + (1-0) = 2;  rows [0, 0] -> 0.
    index = (0, 1, 3, 3): index[1] was 2 at the first visit and is overwritten by the second.
    remainder with buffer_size 10: 6; backtrack + backtrack / 3 * 6 = (0, 6, 0, 3); score 3 + 6."""
    d0 = np.array([[100.0], [1.0], [5.0], [6.0]])
    d1 = np.array([[-50.0], [2.0], [0.0], [5.0]])
    r = R.align(d0, d1, buffer_size=10, cost="squared")
    np.testing.assert_array_equal(r["C"], [[0, INF, INF, INF], [INF, 1, 2, 18], [INF, 10, 26, 2], [INF, 26, 46, 3]])
    np.testing.assert_array_equal(r["index"], [0, 1, 3, 3])
    np.testing.assert_array_equal(r["backtrack_raw"], [0, 2, 0, 1])
    np.testing.assert_array_equal(r["backtrack"], [0, 6, 0, 3])
    assert r["cost"] == 3.0 and r["remainder"] == 6.0 and r["dtw_cost"] == 9.0
    # identical sequences: every step is a free diagonal, and the remainder of an all-zero
    # backtrack is NaN (0 / 0), as in the reference
    r = R.align(d0, d0, buffer_size=10, cost="squared")
    assert r["cost"] == 0.0 and list(r["index"]) == [0, 1, 2, 3] and np.isnan(r["backtrack"]).all()


def test_hand_worked_time_warp_cost():
    """TimeWarpCost (SceneImitateAMP.cpp:5-25), the cost of the reported dtw_cost: rows of two
    points; row a against row b: |(3,4,0)| = 5 and |(0,0,2)| = 2, mean 3.5 (no square: the squared
    distance would be 29); a against itself 0.  The alignment of (., a, a) with (., b, a):
    C(1,1) = 3.5, C(1,2) = 0 + 3.5, C(2,1) = 3.5 + 3.5 = 7, C(2,2) = 0 + min(3.5, 3.5, 7) = 3.5."""
    a = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    b = a + np.array([3.0, 4.0, 0.0, 0.0, 0.0, -2.0])
    val = R.time_warp_cost(np.stack([a, a]), np.stack([b, a]))
    np.testing.assert_array_equal(val, [[3.5, 0.0], [3.5, 0.0]])
    assert R.default_cost(a[None], b[None])[0, 0] == 29.0
    r = R.align(np.stack([9 * a, a, a]), np.stack([-a, b, a]), buffer_size=5)   # "points" is the default
    np.testing.assert_array_equal(r["C"][1:, 1:], [[3.5, 3.5], [7.0, 3.5]])
    # (2,2): preds (3.5, 3.5, 7) tie -> diagonal, backtrack[2] = 0; (1,1): diagonal, backtrack[1] = 3.5
    np.testing.assert_array_equal(r["index"], [0, 1, 2])
    np.testing.assert_array_equal(r["backtrack_raw"], [0, 3.5, 0])
    assert r["dtw_cost"] == 3.5 + 2.0


def test_new_symbols_bound_declared_and_exported(lib):
    declared = _native.header_symbols()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in NEW:
        assert name in _native.SIGNATURES and name in declared and hasattr(raw, name)
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert lib.amx_abi_version() == _native.ABI_VERSION == 2
    assert "#define AMX_ABI_VERSION 2" in open(_native._HEADER).read()


def fake_ctx():
    """A zeroed amx_ctx stand-in: every call below is refused before anything of it is used."""
    buf = (ctypes.c_int * 512)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


D_ = ctypes.c_void_p(4096)  # a non-null dummy: the argument checks never dereference it


def refused(lib, rc, *words):
    assert rc == -1  # AMX_E_ARG
    msg = lib.amx_last_error()
    assert all(w in msg for w in words), msg


def test_alignment_refuses_bad_arguments(lib):
    _keep, ctx = fake_ctx()

    def call(ctx_=ctx, d0=D_, d1=D_, ld=45, dim=45, kind=_native.AMX_DTW_COST_POINTS, n_max=302, lens=(301, 2), len_dev=D_, bs=302, work=D_, cost=D_,
             index=D_, bt=D_, host=True):
        ln = np.asarray(lens, np.int32)
        return lib.amx_dtw_align(ctx_, d0, d1, ld, dim, kind, n_max, ln.ctypes.data if host else None, len_dev, len(ln), bs,
                                 work, cost, None, index, None, bt, None)

    refused(lib, call(ctx_=None), b"amx_dtw_align", b"null context")
    for kw in ("d0", "d1", "len_dev", "work", "cost", "index", "bt"):
        refused(lib, call(**{kw: None}), b"amx_dtw_align", b"null pointer")
    refused(lib, call(host=False), b"amx_dtw_align", b"null pointer")
    refused(lib, call(ld=44), b"amx_dtw_align", b"ld=44 < dim=45")
    refused(lib, call(lens=(301, 1)), b"amx_dtw_align", b"len[1]=1")
    refused(lib, call(lens=(303, 5)), b"amx_dtw_align", b"len[0]=303")
    refused(lib, call(lens=(-4,)), b"amx_dtw_align", b"len[0]=-4")
    refused(lib, call(n_max=1), b"amx_dtw_align", b"n_max=1")
    refused(lib, call(n_max=514), b"amx_dtw_align", b"n_max=514")   # one thread per row of a 512-thread workgroup
    refused(lib, call(dim=0, ld=0), b"amx_dtw_align", b"dim=0")
    refused(lib, call(bs=300), b"amx_dtw_align", b"buffer_size=300 < len[0]=301")
    refused(lib, call(dim=2001, ld=2001), b"amx_dtw_align", b"LDS")
    refused(lib, call(dim=44, ld=44), b"amx_dtw_align", b"cost=1 with dim=44")   # TimeWarpCost needs 3-d points
    refused(lib, call(kind=2), b"amx_dtw_align", b"cost=2")
    assert lib.amx_dtw_work(20, 302) == 20 * 302 * 302
    assert lib.amx_dtw_work(-1, 302) == -1 and lib.amx_dtw_work(4, 1) == -1


def test_row_builders_refuse_bad_arguments(lib):
    _keep, ctx = fake_ctx()   # no character set: d_motion is null
    assert lib.amx_tw_dim(None) == -1 and lib.amx_tw_dim(ctx) == -1
    refused(lib, lib.amx_state_tw_rows(None, D_, 226, 4, 2, D_, 45, None), b"amx_state_tw_rows", b"no character")
    refused(lib, lib.amx_state_tw_rows(ctx, D_, 226, 4, 2, D_, 45, None), b"amx_state_tw_rows", b"no character")
    refused(lib, lib.amx_motion_tw_rows(None, D_, None, 4, 12, 30.0, D_, 45, None), b"amx_motion_tw_rows", b"no motion")
    refused(lib, lib.amx_motion_tw_rows(ctx, D_, None, 4, 12, 30.0, D_, 45, None), b"amx_motion_tw_rows", b"no motion")
