"""The DTW evaluation score of an imitate_amp run, on the device (csrc/amx_dtw.hip).

`evaluate` (milo/milo/utils.py:115-217) ranks policies by `env_infos[-1]['dtw_cost']`, which
gym_deepmimic.py:160-162 takes from DeepMimicCore at the end of an episode: the dynamic-time-
warping cost between the simulated character's trajectory and the kinematic character playing
the reference clip (cSceneImitateAMP::CalcRewardTimeWarp, scenes/SceneImitateAMP.cpp:243-272,
on util/DynamicTimeWarper.cpp), plus one unit per step the episode fell short of the time
warper's buffer.  What the warper compares (BuildTimeWarpData, :537-555: root height and
every joint's world offset from the root joint) can be rebuilt from recorded SimEnv states
alone, so a learned-dynamics rollout is scored here without the physics:

    data0   rows of the trajectory's T + 1 recorded states (`observations` plus the last
            `next_observations`: NewActionUpdate samples the warper before every action, the
            episode end once more, :194-204, 250-260),
    data1   rows of the kinematic character at reset_time + i / update_rate, its root height
            raised by the trajectory's ground-resolve lift (SyncKinCharRoot copies the
            resolved root position to it, scenes/SceneImitate.cpp:550-582) until a looping
            clip starts its next cycle (SyncKinCharNewCycle, :594-607, drops it),
    val     the scene's cell cost TimeWarpCost (SceneImitateAMP.cpp:5-25, passed to the warper
            at :510): the mean over the J points of their Euclidean distance,
    score   C(n-1, n-1) + (buffer_size - n), buffer_size = ceil(update_rate * time_end_max) + 2
            (BuildTimeWarper, :490-513; 302 for the committed args).

Parity with the C++ core is unpinned in two places (it cannot be built here): the sampling
convention of the n = T + 1 rows, and the kinematic character's root height.  The cell cost,
the recurrence, the backtrack and the remainder restate TimeWarpCost and DynamicTimeWarper.cpp
operation for operation, with sums in index order where Eigen's sum() / norm() associate as its
vectorisation decides (tests/dtw_ref.py).  `cost='squared'` selects the warper's DefaultCost
(DynamicTimeWarper.cpp:3-8, a warper built without a cost function) instead: a different
metric, not comparable with recorded 'dtw_cost' values.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from .engine import AmxContext
from .motion import ReferenceMotion


COSTS = {"points": N.AMX_DTW_COST_POINTS, "squared": N.AMX_DTW_COST_SQUARED}


class TimeWarper:
    """cSceneImitateAMP's time warper over a ReferenceMotion: time-warp rows from states and from
    the clip, the batched alignment, and the per-trajectory `dtw_cost`.  Everything stays on the
    device until the caller reads it."""

    def __init__(self, ctx: AmxContext, motion: ReferenceMotion, update_rate: float = 30.0,
                 time_end_max: float = 10.0, cost: str = "points"):
        """`cost`: the cell cost of align / score, 'points' (TimeWarpCost, the scene's: what
        'dtw_cost' means) or 'squared' (the warper's DefaultCost)."""
        if cost not in COSTS:
            raise ValueError(f"TimeWarper: cost must be one of {sorted(COSTS)}, got {cost!r}")
        self.cost = cost
        if not math.isfinite(time_end_max):
            raise ValueError("TimeWarper: time_end_max must be finite (BuildTimeWarper builds no warper otherwise)")
        self.ctx, self.motion = ctx, motion
        self.update_rate = float(update_rate)
        self.buffer_size = int(math.ceil(self.update_rate * float(time_end_max))) + 2
        self.dim = int(ctx.lib.amx_tw_dim(ctx.h))
        if self.dim <= 0:
            raise N.AmxNativeError("TimeWarper: the context has no character (amx_set_motion)")
        self._work = None

    # ---- rows ------------------------------------------------------------------------------------
    def rows_from_states(self, states: torch.Tensor) -> torch.Tensor:
        """[B, dim] time-warp rows of recorded states [B, S] (float64; RecordWorldRootRot only)."""
        if self.motion.flags != 2:
            raise NotImplementedError("time-warp rows from states need RecordWorldRootRot only (humanoid3d_rot_ctrl)")
        c = self.ctx
        s = torch.as_tensor(states, dtype=torch.float64).to(c.device)
        if s.dim() != 2 or s.shape[1] != c.S:
            raise ValueError(f"rows_from_states: states must be [B, {c.S}], got {tuple(s.shape)}")
        if s.stride(1) != 1 or (s.shape[0] > 1 and s.stride(0) < c.S):
            s = s.contiguous()
        out = torch.empty(s.shape[0], self.dim, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_state_tw_rows(c.h, s.data_ptr(), s.stride(0) if s.shape[0] > 1 else c.S, s.shape[0],
                                        self.motion.flags, out.data_ptr(), self.dim, c.stream), "amx_state_tw_rows")
        return out

    def rows_from_motion(self, t0, n: int, lift=None) -> torch.Tensor:
        """Rows of the kinematic character from clip time t0 on, one per 1 / update_rate: [n, dim]
        for a scalar t0, [T, n, dim] for T start times; `lift` (scalar or [T]) is added to the root
        height (the trajectory's ground-resolve lift; None: 0) for the rows of the cycle the
        trajectory was reset in."""
        c = self.ctx
        scalar = t0.dim() == 0 if isinstance(t0, torch.Tensor) else np.ndim(t0) == 0
        t = torch.as_tensor(t0, dtype=torch.float64).reshape(-1).to(c.device).contiguous()
        T = t.numel()
        lf = None
        if lift is not None:
            lf = torch.as_tensor(lift, dtype=torch.float64).reshape(-1).to(c.device)
            lf = lf.expand(T).contiguous() if lf.numel() == 1 else lf.contiguous()
            if lf.numel() != T:
                raise ValueError(f"rows_from_motion: {lf.numel()} lifts for {T} start times")
        out = torch.empty(T, int(n), self.dim, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_motion_tw_rows(c.h, t.data_ptr(), N.ptr(lf), T, int(n), self.update_rate, out.data_ptr(),
                                         self.dim, c.stream), "amx_motion_tw_rows")
        return out[0] if scalar else out

    # ---- alignment -------------------------------------------------------------------------------
    def align(self, data0: torch.Tensor, data1: torch.Tensor, lengths, buffer_size: int | None = None,
              cost: str | None = None) -> dict:
        """The raw alignment of T row sequences: data0 / data1 [T, n_max, dim] (or [n, dim] for
        one), trajectory t using its first lengths[t] rows of both.  Returns device tensors: cost
        [T] = C(n-1, n-1), dtw_cost [T] = cost + (buffer_size - n), index [T, n_max] int32,
        backtrack [T, n_max] (remainder applied) and backtrack_raw (before it); entries past a
        trajectory's length are zero.  `cost`: 'points' / 'squared' (None: the warper's own)."""
        kind = COSTS[self.cost if cost is None else cost]
        c = self.ctx
        d0 = torch.as_tensor(data0, dtype=torch.float64).to(c.device)
        d1 = torch.as_tensor(data1, dtype=torch.float64).to(c.device)
        if d0.dim() == 2:
            d0, d1 = d0[None], d1[None]
        d0, d1 = d0.contiguous(), d1.contiguous()
        if d0.shape != d1.shape or d0.dim() != 3:
            raise ValueError(f"align: data0 {tuple(d0.shape)} and data1 {tuple(d1.shape)} must be equal [T, n_max, dim]")
        T, n_max, dim = d0.shape
        ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1), dtype=np.int32)
        if ln.size != T:
            raise ValueError(f"align: {ln.size} lengths for {T} trajectories")
        bs = int(n_max if buffer_size is None else buffer_size)
        need = int(c.lib.amx_dtw_work(T, n_max))
        if need < 0:
            raise ValueError(f"align: T={T}, n_max={n_max}")
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(max(need, 1), dtype=torch.float64, device=c.device)
        ln_dev = torch.from_numpy(ln).to(c.device)
        cost = torch.empty(T, dtype=torch.float64, device=c.device)
        dtw = torch.empty(T, dtype=torch.float64, device=c.device)
        index = torch.zeros(T, n_max, dtype=torch.int32, device=c.device)
        raw = torch.zeros(T, n_max, dtype=torch.float64, device=c.device)
        bt = torch.zeros(T, n_max, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_dtw_align(c.h, d0.data_ptr(), d1.data_ptr(), dim, dim, kind, n_max, ln.ctypes.data,
                                    ln_dev.data_ptr(), T, bs, self._work.data_ptr(), cost.data_ptr(), dtw.data_ptr(),
                                    index.data_ptr(), raw.data_ptr(), bt.data_ptr(), c.stream), "amx_dtw_align")
        return dict(cost=cost, dtw_cost=dtw, index=index, backtrack=bt, backtrack_raw=raw)

    # ---- scores ----------------------------------------------------------------------------------
    def score(self, states_list, reset_times) -> dict:
        """`dtw_cost` of T trajectories: states_list[t] the trajectory's T_t + 1 recorded states
        ([T_t + 1, S]: `observations` plus the last `next_observations`), reset_times[t] the clip
        time it was reset at.  Returns dtw_cost [T] (device), and per trajectory the backtrack
        (per-state costs, remainder included) and the index path, cut to its length."""
        c = self.ctx
        T = len(states_list)
        t0 = torch.as_tensor(np.asarray(reset_times, dtype=np.float64).reshape(-1)).to(c.device)
        if T == 0 or t0.numel() != T:
            raise ValueError(f"score: {T} trajectories, {t0.numel()} reset times")
        sl = [torch.as_tensor(s, dtype=torch.float64).to(c.device) for s in states_list]
        ln = [int(s.shape[0]) for s in sl]
        n_max = self.buffer_size
        if max(ln) > n_max or min(ln) < 2:
            raise ValueError(f"score: trajectories of {min(ln)}..{max(ln)} states; the warper holds 2..{n_max}")
        rows = self.rows_from_states(torch.cat(sl, dim=0))
        starts = np.cumsum(ln) - np.asarray(ln)
        dst = np.concatenate([t * n_max + np.arange(n) for t, n in enumerate(ln)])
        data0 = torch.zeros(T * n_max, self.dim, dtype=torch.float64, device=c.device)
        data0[torch.from_numpy(dst).to(c.device)] = rows
        # the kinematic character's root height: the clip's plus this trajectory's reset lift
        lift = None
        if self.motion.resolve:
            s0 = rows[torch.from_numpy(starts).to(c.device), 1]
            lift = s0 - self.rows_from_motion(t0, 1)[:, 0, 1]
        data1 = self.rows_from_motion(t0, n_max, lift)
        r = self.align(data0.view(T, n_max, self.dim), data1, ln, buffer_size=n_max)
        return dict(dtw_cost=r["dtw_cost"], cost=r["cost"],
                    backtrack=[r["backtrack"][t, :n] for t, n in enumerate(ln)],
                    index=[r["index"][t, :n] for t, n in enumerate(ln)])

    def score_paths(self, paths) -> dict:
        """score() of path dicts that carry `reset_time` (sample_points(..., dtw=...) sets it)."""
        states = [np.concatenate([p["observations"], p["next_observations"][-1:]], axis=0) for p in paths]
        return self.score(states, [float(p["reset_time"]) for p in paths])
