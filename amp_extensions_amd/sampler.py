"""`sample_points` drop-in (milo/milo/sampler.py:87-130) over the GPU lane engine.

Reference contract (sampler.py:8-84, 112-130): W workers; worker i has quota q = ceil(N / W)
and collects complete trajectories one after another until it holds >= q samples (mode
'samples') or q trajectories (mode 'trajectories').  Trajectory j = 1, 2, ... of worker i is
seeded with s_ij = 12345 + base_seed * i + j: `env.seed_env(s_ij)` then `env.reset()` draws the
reset time t ~ U(0, time_max) from gym's np_random, and `np.random.seed(s_ij)` seeds the
policy's per-step draws (np.random.uniform() for the eps test, then randn(A)); the env's
reset counter makes trajectory j run on ensemble member j mod M.  The result lists worker
0's paths in order, then worker 1's, ...

Here a worker's trajectories run concurrently on GPU lanes.  Every trajectory is
exact-seeded (its reset time, noise and ensemble member depend only on (i, j)), so they can
run in any order and concurrency: trajectory j of worker i is admitted while the lengths its
predecessors have reached so far sum to less than q (a lower bound on the sum that decides
whether j is needed), dropped as soon as that bound reaches q, and the result is exactly
trajectories 1..n_i of the sequential reference, n_i = min{n : sum_{j <= n} len_j >= q}
('trajectories' mode: the first q).  How many run at once is set by an estimate of the
lengths still to come (the horizon R: the reference's worst case; or, speculatively, the
mean length of the trajectories ended so far), see _Admission.  With rng='reference' every
trajectory's reset time and noise come from the reference's own seeds (the PCG64 reset draw
per trajectory; the MT19937 policy noise from per-lane generators in the HIP library's host
code, amx_mt_policy_noise, uploaded per chunk), so the output equals the reference's paths up
to the ensemble's fp32 arithmetic; rng='device' draws them from Philox on the GPU (same
structure and admission, different random streams, no host RNG work).

Lanes: W * ceil(q / R) lanes suffice for the worst-case rule (x4 with speculation), capped by
the env's lane count.  Steps run in chunks of K synchronous steps between host decisions,
replayed as one captured HIP graph per chunk; a lane whose trajectory ends inside a chunk
idles to its end.  The transitions of in-flight lanes are compacted on the device after every
chunk (one index gather into a transition store) and the store is reordered into path order
and copied to the host ONCE at the end; each path's arrays are views of that copy.
"""
from __future__ import annotations

import gc
import math
import threading
import time
import weakref

import numpy as np
import torch

from . import _native as N
from .rollout import RolloutEngine
from .sim_env import BatchedSimEnv


def _gym_np_random(seed: int) -> np.random.Generator:
    """gym 0.26.1 seeding.np_random(seed) (environment.yml:123): Generator(PCG64(SeedSequence))."""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


class _Traj:
    __slots__ = ("worker", "j", "seed", "lane", "length", "ended", "segs", "reset_time")

    def __init__(self, worker: int, j: int, seed: int):
        self.worker, self.j, self.seed = worker, j, seed
        self.lane = -1
        self.length = 0       # transitions so far (the final length once ended)
        self.ended = False
        self.segs = []  # (store row, count) pieces in step order
        self.reset_time = None  # the clip time (table row) its reset drew, where the host knows it


class _Store:
    """Device transition store (compacted lane rows), grown geometrically."""

    def __init__(self, dev, S: int, A: int, cap: int):
        self.dev, self.S, self.A, self.n = dev, S, A, 0
        self._alloc(max(cap, 1024))

    def _alloc(self, cap: int):
        old = getattr(self, "obs", None)
        z = lambda w, dt: torch.empty(cap, w, dtype=dt, device=self.dev)
        new = (z(self.S, torch.float64), z(self.S, torch.float64), z(self.A, torch.float64), z(self.A, torch.float32))
        if old is not None:
            for dst, src in zip(new, (self.obs, self.nxt, self.act, self.mean)):
                dst[:self.n].copy_(src[:self.n])
        self.obs, self.nxt, self.act, self.mean = new
        self.cap = cap

    def append_from(self, src, idx: torch.Tensor) -> int:
        """Rows idx of the flat [K * L] chunk arrays src = (obs, next_obs, acts, means)."""
        m = idx.numel()
        if self.n + m > self.cap:
            self._alloc(max(2 * self.cap, self.n + m))
        s = slice(self.n, self.n + m)
        for dst, x in zip((self.obs, self.nxt, self.act, self.mean), src):
            torch.index_select(x, 0, idx, out=dst[s])
        base = self.n
        self.n += m
        return base


class _FreeLanes:
    """The idle lanes.  Member-blocked engines (RolloutEngine.member_blocks = Bq: lane b runs
    member b // Bq only) keep one list per member: trajectory j resets to member j mod M
    (sim_env.py:282-283 with the counter at j - 1), so it takes a lane of that block."""

    def __init__(self, L: int, M: int, Bq: int):
        self.M, self.Bq = M, Bq
        if Bq:
            self.lists = [list(range((g + 1) * Bq - 1, g * Bq - 1, -1)) for g in range(M)]
        else:
            self.lists = [list(range(L - 1, -1, -1))]

    def __bool__(self) -> bool:
        return any(self.lists)

    def take(self, j: int) -> int:
        """A lane for trajectory j (-1: none of its member's block is free)."""
        lst = self.lists[j % self.M if self.Bq else 0]
        return lst.pop() if lst else -1

    def put(self, lane: int) -> None:
        self.lists[lane // self.Bq if self.Bq else 0].append(lane)


class _Admission:
    """Which trajectory runs on which lane: the host-side state of one sample_points call (plain
    Python: no torch, no engine, no device).

    A worker's trajectories are admitted in seed order j.  Trajectory j is needed iff the exact
    lengths of 1..j-1 sum to less than the quota q; the lengths reached so far give a lower bound
    LB_j of that sum, so j is admitted only while LB_j < q and an in-flight trajectory whose
    LB_j >= q is provably not needed and is dropped (its lane freed).  Among admissible
    trajectories the concurrency is capped by an estimate: sum over the admitted of (final length,
    or max(length so far, L^)) < q, with L^ = the horizon R (speculate=False: the reference's
    worst case, never wasted work) or the mean length of the trajectories ended so far
    (speculate=True: short trajectories admit more at once; any surplus trajectory completes or is
    dropped and never enters the result).  Each trajectory is exact-seeded, so its transitions do
    not depend on when or on which lane it ran: the result is trajectories 1..n_i of every worker,
    n_i = min{n : sum_{j <= n} len_j >= q}, for any admission order and any lag between a chunk's
    launch and its advance()."""

    def __init__(self, W: int, quota: int, mode: str, base_seed: int, R: int, speculate: bool, L: int, M: int,
                 Bq: int):
        self.W, self.quota, self.mode, self.base_seed, self.R, self.speculate = W, quota, mode, base_seed, R, speculate
        self.adm: list[list[_Traj]] = [[] for _ in range(W)]   # admitted trajectories, in j order
        self.next_j = [1] * W
        self.done_w = [False] * W
        self.lane_tr: list[_Traj | None] = [None] * L
        self.free = _FreeLanes(L, M, Bq)
        self.ended_sum, self.ended_n = 0, 0

    def _drop(self, tr: _Traj) -> None:
        if tr.lane >= 0:
            self.lane_tr[tr.lane] = None
            self.free.put(tr.lane)
            tr.lane = -1

    def admit(self) -> list[_Traj]:
        """Per worker: drop the unneeded, detect completion, admit (round-robin).  Returns the
        newly admitted trajectories, each on its lane."""
        W, quota, mode, adm, done_w, free = self.W, self.quota, self.mode, self.adm, self.done_w, self.free
        # speculation: 2x the worst-case concurrency until lengths are known (lanes are nearly free
        # at these counts: the step time is latency-bound), then the mean ended length
        lhat = (float(self.R) if not self.speculate
                else (self.ended_sum / self.ended_n if self.ended_n >= 4 else 0.5 * self.R))
        for w in range(W):
            if done_w[w]:
                continue
            trs = adm[w]
            if mode == "samples":
                lb, cut = 0, len(trs)
                for i, tr in enumerate(trs):
                    if lb >= quota:
                        cut = i
                        break
                    lb += tr.length
                for tr in trs[cut:]:
                    self._drop(tr)
                del trs[cut:]
                if trs and all(tr.ended for tr in trs) and sum(tr.length for tr in trs) >= quota:
                    done_w[w] = True
            elif len(trs) == quota and all(tr.ended for tr in trs):
                done_w[w] = True
        new = []
        # per worker: the lower bound (lengths so far) and the estimate, summed once per chunk
        # and extended as trajectories are admitted (a new one adds 0 and lhat)
        lbs, ests = [0] * W, [0.0] * W
        if mode == "samples":
            for w in range(W):
                if not done_w[w]:
                    lbs[w] = sum(tr.length for tr in adm[w])
                    ests[w] = sum(tr.length if tr.ended else max(tr.length, lhat) for tr in adm[w])
        progress = True
        while free and progress:
            progress = False
            for w in range(W):
                if not free or done_w[w]:
                    continue
                trs = adm[w]
                ok = (lbs[w] < quota and ests[w] < quota) if mode == "samples" else len(trs) < quota
                if ok:
                    j = self.next_j[w]
                    lane = free.take(j)
                    if lane < 0:  # (member-blocked: j waits for a lane of its member's block)
                        continue
                    self.next_j[w] += 1
                    tr = _Traj(w, j, 12345 + self.base_seed * w + j)
                    tr.lane = lane
                    self.lane_tr[tr.lane] = tr
                    trs.append(tr)
                    new.append(tr)
                    ests[w] += max(0, lhat)
                    progress = True
        return new

    def in_flight(self) -> list[tuple[int, _Traj]]:
        """The (lane, trajectory) pairs of the active lanes, in lane order."""
        return [(b, tr) for b, tr in enumerate(self.lane_tr) if tr is not None]

    def live(self, launched: list[tuple[int, _Traj]]) -> list[tuple[int, _Traj]]:
        """Of the pairs a chunk was launched with, those whose trajectory is still running on its
        lane (not ended in an earlier chunk, not dropped): the ones the chunk's steps belong to."""
        return [(b, tr) for b, tr in launched if not tr.ended and tr.lane == b]

    def advance(self, live: list[tuple[int, _Traj]], n, hit, rows) -> None:
        """A chunk's outcome for its live() pairs: pair i ran n[i] more steps, kept at store row
        rows[i] on, and ended iff hit[i] (its lane is freed)."""
        for (_, tr), n_i, h, row in zip(live, n.tolist(), hit.tolist(), rows.tolist()):
            tr.segs.append((row, n_i))
            tr.length += n_i
            if h:
                tr.ended = True
                self.ended_sum += tr.length
                self.ended_n += 1
                self._drop(tr)

    def trajectories(self) -> list[_Traj]:
        """The result, in (worker, j) order."""
        return [tr for trs in self.adm for tr in trs]


def _chunk_rows(done: np.ndarray, lanes: np.ndarray, L: int):
    """done [K, n] (bool) of the n lanes `lanes` over a chunk's K steps of L lanes -> per lane the
    steps it ran (through its first done step; K if none) and whether it ended, and for the
    compacted rows (lane after lane, each in step order) every lane's first row `starts` and the
    rows' indices step * L + lane into the flat [K * L] chunk arrays."""
    hit = done.any(axis=0)
    n = np.where(hit, done.argmax(axis=0) + 1, done.shape[0])
    starts = np.cumsum(n) - n
    step_of = np.arange(int(n.sum())) - np.repeat(starts, n)
    return n, hit, starts, step_of * L + np.repeat(lanes, n)


def _reset_time_max(env) -> float:
    """The reset-time window [0, time_max) every trajectory's env.reset() draws from
    (sim_env.py:76-77, 276): reset_args['time_max'] when custom_time is on, else the clip length
    (a reset table: its length in rows).  A BatchedSimEnv keeps its reset_args; a RolloutEngine
    its reset_time_max (0: the whole source)."""
    src = env.engine if isinstance(env, BatchedSimEnv) else env
    ra = getattr(env, "reset_args", None)
    if ra is not None and ra.get("custom_time"):
        return float(ra["time_max"])
    if float(getattr(src, "reset_time_max", 0.0) or 0.0) > 0.0:
        return float(src.reset_time_max)
    return src.motion.get_motion_length() if src.motion is not None else float(src.table.shape[0])


def _sampler_engine(env, lanes: int, K: int, policy, time_max: float, member_blocks: int = 0) -> RolloutEngine:
    """A lanes-sized engine on the env's ensemble, reset source and termination (cached per
    lane count, chunk, reset window and member blocking); its device-drawn motion resets use the
    env's window.  member_blocks = Bq > 0: lanes = M * Bq, lane b steps through member b // Bq
    only (RolloutEngine.member_blocks)."""
    src = env.engine if isinstance(env, BatchedSimEnv) else env
    cache = src.__dict__.setdefault("_sampler_engines", {})
    key = (lanes, K, float(time_max), int(member_blocks))
    eng = cache.get(key)
    if eng is None:
        reset_source = src.motion if src.motion is not None else src.table
        eng = RolloutEngine(src.ens, reset_source, lanes=lanes, term=src.term, policy=policy, seed=src.seed,
                            max_steps=K, auto_reset=False, record_means=True)
        # (0 = the whole clip; a table source is already cut to the window's rows)
        if src.motion is not None and time_max != src.motion.get_motion_length():
            eng.reset_time_max = float(time_max)
        eng.member_blocks = int(member_blocks)
        cache[key] = eng
    # the env's reset_args noise (AddNoise) as it is NOW: a later set_reset_noise on the env
    # reaches the cached engine.  The noise draws come from Philox(engine seed; lane, reset#),
    # not from the trajectory seed, so with noise on, sample_points' paths depend on the lane
    # count and the admission order (the reference's own gRand stream is seeded from the wall
    # clock, util/Rand.cpp:8-9, so it is not reproducible either).
    eng._reset_noise = getattr(src, "_reset_noise", None)
    eng.policy = policy
    return eng


def _mjrl_fingerprint(policy) -> tuple:
    """The VALUES of every trainable tensor of an mjrl MLP (≈8.6 k floats at S = 197, a 34 KB
    copy per sample_points call).  Identities and version counters are not enough:
    set_param_values rebinds param.data (gaussian_mlp.py:67-85), but an optimizer step updates
    in place (behavior_cloning.py:125-132) and `p.data.add_()` / `p.data.copy_()` go through a
    `.data` alias whose version counter is not the parameter's, so only the values see every
    kind of update."""
    ts = [p.detach() for p in policy.model.parameters()] + [policy.log_std.detach()]
    vals = torch.cat([t.reshape(-1).to("cpu", torch.float64) for t in ts])
    return vals, np.asarray(policy.log_std_val).tobytes()


def _same_fingerprint(a: tuple, b: tuple) -> bool:
    return a[1] == b[1] and a[0].shape == b[0].shape and torch.equal(a[0], b[0])


def device_policy(env, policy):
    """`policy` as the sampler's DevicePolicy.  A DevicePolicy passes through; the reference's
    mjrl `MLP` (gaussian_mlp.py:7-104: `model.fc_layers`, `log_std`, `log_std_val`) is wrapped
    once (DevicePolicy.from_mjrl, cached on the object) and re-synced whenever its parameters
    changed since the last call, so batch_reinforce.py:88-90 passes its own policy unchanged."""
    from .policy import DevicePolicy
    if isinstance(policy, DevicePolicy):
        return policy
    model = getattr(policy, "model", None)
    if model is None or not hasattr(model, "fc_layers") or not hasattr(policy, "log_std"):
        raise TypeError(f"sample_points: policy must be a DevicePolicy or an mjrl MLP, got {type(policy).__name__}")
    if float(getattr(policy, "eps", 0.0) or 0.0) != 0.0:
        raise NotImplementedError("sample_points: mjrl MLP with eps > 0 (uniform random actions) is not supported")
    src = env.engine if isinstance(env, BatchedSimEnv) else env
    ctx = src.ctx
    fp = _mjrl_fingerprint(policy)
    cached = policy.__dict__.get("_amx_device_policy")
    if cached is None or cached[0] is not ctx:
        dp = DevicePolicy.from_mjrl(ctx, policy)
        policy.__dict__["_amx_device_policy"] = (ctx, dp, fp)
        return dp
    _, dp, old = cached
    if not _same_fingerprint(old, fp):
        dp.sync_from([(l.weight.data, l.bias.data) for l in policy.model.fc_layers],
                     np.asarray(policy.log_std_val, np.float64))
        policy.__dict__["_amx_device_policy"] = (ctx, dp, fp)
    return dp


class _HostNoise:
    """Per-lane numpy-legacy MT19937 generators of the reference policy noise, advanced in the
    HIP library's host code (amx_mt_seed / amx_mt_policy_noise: bit-exact with
    np.random.seed(s); [np.random.uniform(); np.random.randn(A)] per step) into a pinned
    [K, L, A] buffer, one call per chunk for all lanes in flight."""

    def __init__(self, lib, L: int, K: int, A: int):
        self.lib, self.L, self.K, self.A = lib, L, K, A
        self.states = np.zeros((L, N.AMX_MT_STATE_BYTES), np.uint8)
        # pinned buffers, chunk c's in bufs[c % 3]: the next chunk's noise is drawn into one while
        # another's upload and the current chunk's steps run on the GPU (three: pipelined, chunk
        # c + 1's draw starts before chunk c - 1 has been read back)
        pin = torch.cuda.is_available()
        self.bufs = [torch.zeros(K, L, A, dtype=torch.float64, pin_memory=pin) for _ in range(3)]
        self._thread, self._err = None, None

    def seed(self, lanes: np.ndarray, seeds: np.ndarray) -> None:
        sl = np.ascontiguousarray(lanes, np.int32)
        sd = np.asarray(seeds, np.int64)
        if sd.size and (sd.min() < 0 or sd.max() >= 2 ** 32):  # np.random.seed's own range check
            raise ValueError(f"Seed must be between 0 and 2**32 - 1 (sample_points trajectory seeds {sd.min()}..{sd.max()})")
        sd = np.ascontiguousarray(sd, np.uint32)
        N.check(self.lib.amx_mt_seed(self.states.ctypes.data, self.L, sl.ctypes.data, sd.ctypes.data, sl.size),
                "amx_mt_seed")

    def draw(self, lanes: np.ndarray, buf: torch.Tensor) -> torch.Tensor:
        """The next K steps' noise of `lanes` into their slots of `buf` (other slots untouched)."""
        sl = np.ascontiguousarray(lanes, np.int32)
        N.check(self.lib.amx_mt_policy_noise(self.states.ctypes.data, self.L, sl.ctypes.data, sl.size, self.K,
                                             self.A, buf.data_ptr(), self.L * self.A, self.A),
                "amx_mt_policy_noise")
        return buf

    def draw_ahead(self, lanes: np.ndarray, which: int, background: bool) -> None:
        """The next chunk's noise of the lanes in flight into bufs[which], while the GPU steps.
        background (the pipelined collector): on a host thread (the ctypes call releases the GIL)
        while the main thread reads the previous chunk and admits; join() before any seed or
        draw touches the generator states."""
        if not background:
            self.draw(lanes, self.bufs[which])
            return
        self.join()
        self._err = None

        def run():
            try:
                self.draw(lanes, self.bufs[which])
            except BaseException as e:  # re-raised by join()
                self._err = e
        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()

    def join(self) -> None:
        th = self._thread
        if th is not None:
            th.join()
            self._thread = None
            if self._err is not None:
                raise self._err


class _ChunkGraph:
    """The K synchronous steps of a chunk captured once as a HIP graph (the lanes' resets and
    the noise upload stay outside, on the same stream), so a chunk costs one replay instead of
    ~8 launches per step from Python."""

    def __init__(self, eng: RolloutEngine, K: int, noise_dev):
        c = eng.ctx
        # (a weak reference: the graph is cached on the engine, engine -> graph -> engine would be
        # a reference cycle that only the garbage collector frees)
        self.eng, self.K = weakref.proxy(eng), K
        self.g = torch.cuda.CUDAGraph()
        eng.sync_step_counter(to_device=True)
        side = torch.cuda.Stream(c.device)
        side.wait_stream(torch.cuda.current_stream(c.device))
        t0 = eng.t
        # no garbage collection during the capture: a collected cycle holding another graph or
        # device memory would be torn down in the middle of it (a HIP error / abort).  One
        # collection up front (torch.cuda.graph does the same), then the collector is off until
        # capture_end.  (capture_begin/end directly: torch.cuda.graph's context manager also
        # synchronises and empties the allocator cache, 13 ms per capture)
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        with torch.cuda.stream(side):
            eng._capturing = True
            self.g.capture_begin(capture_error_mode="thread_local")
            try:
                for k in range(K):
                    eng.step(noise=None if noise_dev is None else noise_dev[k])
                N.check(c.lib.amx_counter_add(c.h, eng.dev_step.data_ptr(), K, c.stream), "amx_counter_add")
            finally:
                self.g.capture_end()
                eng._capturing = False
                if gc_was_on:
                    gc.enable()
        torch.cuda.current_stream(c.device).wait_stream(side)
        eng.t, eng.step_counter = t0, eng.step_counter - K  # the captured steps did not run
        eng._graph_ahead = True

    def replay(self) -> None:
        self.g.replay()
        self.eng.t = self.K
        self.eng.step_counter += self.K
        self.eng._graph_ahead = True


# The device rows of the last sample_points call, in path order, beside the read-only host
# arrays they were copied to: relabel_paths (relabel.py:_device_rows) reads them instead of
# uploading the same bytes back when its paths are views of those host arrays.  One entry (the
# newest call); the host arrays are read-only, so the two copies cannot diverge.
_last_rows: dict = {}


def _to_host_path_order(perm: torch.Tensor, arrays, wait: bool = True):
    """The store's rows gathered into path order on the device, then ONE copy each into pinned
    host memory (2-4x the pageable .cpu() rate; torch's pinned-block cache reuses the blocks of
    paths the caller has dropped).  The returned numpy arrays keep their pinned tensors alive and
    are read-only (the reference's own code only reads the paths' arrays); the device rows of
    (observations, next observations, actions) stay registered in _last_rows.  wait=False:
    returns (arrays, event) with the copies still in flight (the event completes them)."""
    sel = [x.index_select(0, perm) for x in arrays]
    pin = torch.cuda.is_available()
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=pin) for t in sel]
    for h, t in zip(host, sel):
        h.copy_(t, non_blocking=pin)
    ev = None
    if pin:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(sel[0].device))
        if wait:
            ev.synchronize()
    out = [h.numpy() for h in host]
    for a in out:
        a.flags.writeable = False
    _last_rows.clear()
    _last_rows.update(observations=(out[0], sel[0]), next_observations=(out[1], sel[1]), actions=(out[2], sel[2]))
    return out if wait else (out, ev)


def _build_paths(trajs, store, eng: RolloutEngine, dev):
    """The trajectories' transitions in path order: one device gather, one asynchronous copy
    into pinned host memory, the path dicts built as views while it runs."""
    segs = [seg for tr in trajs for seg in tr.segs]
    starts = np.fromiter((b for b, _ in segs), np.int64, len(segs))
    lens = np.fromiter((n for _, n in segs), np.int64, len(segs))
    total = int(lens.sum())
    perm = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
    pd = torch.from_numpy(perm).to(dev)
    host, copied = _to_host_path_order(pd, (store.obs, store.nxt, store.act, store.mean), wait=False)
    log_std = np.asarray(eng.policy.log_std_val, dtype=np.float64)
    # every step's log_std row (gaussian_mlp.py:102) as read-only broadcast views of one row
    ls_rows = np.broadcast_to(log_std, (total, log_std.shape[-1]))
    paths, off = [], 0
    for tr in trajs:
        T = tr.length
        sl = slice(off, off + T)
        m = host[3][sl]
        paths.append(dict(observations=host[0][sl], next_observations=host[1][sl], actions=host[2][sl],
                          rewards=np.zeros(T, dtype=np.int64),
                          agent_infos=dict(mean=m, log_std=ls_rows[sl], evaluation=m),
                          env_infos=[{} for _ in range(T)], terminated=True))
        off += T
    if copied is not None:
        copied.synchronize()
    return paths, off


def _deliver_dtw(dtw, trajs, paths) -> None:
    """The evaluation's deliveries (gym_deepmimic.py:160-162): path['reset_time'] and the last
    env_info's 'dtw_cost', scored in one launch from the device rows the paths were copied from."""
    obs, nxt = _last_rows["observations"][1], _last_rows["next_observations"][1]
    states, off = [], 0
    for tr in trajs:
        states.append(torch.cat([obs[off:off + tr.length], nxt[off + tr.length - 1:off + tr.length]], dim=0))
        off += tr.length
    cost = dtw.score(states, [tr.reset_time for tr in trajs])["dtw_cost"].cpu().numpy()
    for tr, p, c in zip(trajs, paths, cost):
        p["reset_time"] = tr.reset_time
        p["env_infos"][-1]["dtw_cost"] = float(c)


def _chunk_graph(eng: RolloutEngine, K: int, noise_dev, eval_mode: bool) -> _ChunkGraph:
    """The chunk's captured graph, cached on the engine across sample_points calls: it bakes in
    the engine's and the policy's device buffers (persistent; DevicePolicy.sync_from rewrites
    them in place), the noise buffer, eval_mode and, for device-drawn noise, the policy seed."""
    pol = eng.policy
    key = (K, 0 if noise_dev is None else noise_dev.data_ptr(), bool(eval_mode), id(pol), pol.blob.data_ptr(),
           pol.noise_scale.data_ptr(), pol.H1, pol.H2, pol.seed if noise_dev is None else 0, bool(eng.fuse_assembly))
    cache = eng.__dict__.setdefault("_chunk_graphs", {})
    g = cache.get(key)
    if g is None:
        if len(cache) >= 4:  # (re-created policies: keep the newest few)
            cache.pop(next(iter(cache)))
        eng.begin_rollout()
        g = cache[key] = _ChunkGraph(eng, K, noise_dev)
    else:
        eng.begin_rollout()
        eng.sync_step_counter()
    return g


def _noise_buffer(eng: RolloutEngine, K: int, L: int, A: int) -> torch.Tensor:
    """The [K, L, A] device buffer of the uploaded reference noise (persistent per engine: the
    cached chunk graphs read it)."""
    buf = eng.__dict__.get("_noise_dev")
    if buf is None or tuple(buf.shape) != (K, L, A):
        buf = eng.__dict__["_noise_dev"] = torch.zeros(K, L, A, dtype=torch.float64, device=eng.ctx.device)
    return buf


def _chunk_arrays(eng: RolloutEngine, K: int):
    """The engine's records (obs, next_obs, acts, means) of a chunk's K steps as flat [K * L] rows."""
    m = K * eng.B
    return tuple(x[:K].reshape(m, x.shape[-1]) for x in (eng.obs, eng.next_obs, eng.acts, eng.means))


class _ChunkRing:
    """Two device copies of a chunk's K x L transitions: chunk i is copied into slot i % 2 right
    after its steps (no host information needed), so chunk i + 1 can be queued before chunk i's
    done flags are read; chunk i's rows are compacted from its slot one iteration later."""

    def __init__(self, eng: RolloutEngine, K: int):
        self.slots = [tuple(torch.empty_like(x) for x in _chunk_arrays(eng, K)) for _ in range(2)]
        self.K = K

    def snapshot(self, eng: RolloutEngine, si: int) -> None:
        for dst, src in zip(self.slots[si], _chunk_arrays(eng, self.K)):
            dst.copy_(src)


class _Stage:
    """One set of pinned host staging for a chunk: its reset inputs and, with read_back (the
    pipelined collector), its done flags, the event of their copy and its compaction indices."""

    def __init__(self, L: int, K: int, rows_dtype, dev, read_back: bool):
        pin = torch.cuda.is_available()
        self.mask = torch.zeros(L, dtype=torch.uint8, pin_memory=pin)
        self.counts = torch.zeros(L, dtype=torch.int32, pin_memory=pin)
        self.rows = torch.zeros(L, dtype=rows_dtype, pin_memory=pin)
        if read_back:
            self.done = torch.zeros(K, L, dtype=torch.uint8, pin_memory=pin)
            self.event = torch.cuda.Event() if pin else None
            self.flat = torch.zeros(K * L, dtype=torch.int64, pin_memory=pin)
            self.flat_dev = torch.empty(K * L, dtype=torch.int64, device=dev)


def _reset_lanes(eng: RolloutEngine, st: _Stage, devs, active: np.ndarray, new: list, rng: str,
                 time_max: float, t_out: torch.Tensor | None = None) -> None:
    """A chunk's resets: the new trajectories' lanes (reset counter j - 1 -> member j mod M; with
    rng='reference' at the reset time drawn from the trajectory's seed) and the idle lanes, staged
    in `st` and uploaded into devs = (mask, counts, rows) without a host wait.  t_out ([L] float64,
    the DTW score's request with rng='device'): the times the device drew are read back into the
    new trajectories (one host wait)."""
    mask_dev, counts_dev, rows_dev = devs
    mask_np, counts_np, rows_np = st.mask.numpy(), st.counts.numpy(), st.rows.numpy()
    eng.begin_rollout()
    mask_np.fill(1)
    mask_np[active] = 0
    counts_np.fill(0)
    for tr in new:
        mask_np[tr.lane] = 1
        counts_np[tr.lane] = tr.j - 1
        if rng == "reference":
            t = _gym_np_random(tr.seed).uniform(low=0, high=time_max)  # seed_env + reset (sim_env.py:132,276)
            rows_np[tr.lane] = t if eng.motion is not None else int(np.floor(t))
            tr.reset_time = float(t)
    mask_dev.copy_(st.mask, non_blocking=True)
    counts_dev.copy_(st.counts, non_blocking=True)
    # reset lanes restart their counter at j - 1 (idle lanes at 0); the reset kernel adds one
    torch.where(mask_dev.bool(), counts_dev, eng.reset_count, out=eng.reset_count)
    if rng == "reference":
        rows_dev.copy_(st.rows, non_blocking=True)
    eng.reset_lanes(mask_dev, rows_dev if rng == "reference" else None, t_out=t_out)
    if t_out is not None and rng != "reference" and new:
        drawn = t_out.cpu().numpy()
        for tr in new:
            tr.reset_time = float(drawn[tr.lane])


def _collect(eng: RolloutEngine, W: int, quota: int, mode: str, base_seed: int, rng: str, eval_mode: bool,
             time_max: float, speculate: bool = True, graph: bool = True, pipeline: bool = True, dtw=None):
    """Run the W workers' trajectory sequences on the engine's lanes (see the module notes and
    _Admission): admit, launch a chunk (resets, noise, the K steps), read a chunk back (its done
    flags; its in-flight rows compacted into the store; its trajectories advanced).

    pipeline=False reads chunk i back before chunk i + 1 is queued: one blocking read of the done
    flags per chunk, the rows compacted straight from the engine's buffers.  pipeline=True keeps
    the host one chunk behind the GPU: chunk i is queued (with a raw copy of its transitions and an
    async copy of its done flags) before chunk i-1 is read back.  Admission then sees the results
    through chunk i-2: a lane whose trajectory ended in chunk i-1 runs chunk i idle (its steps are
    never attributed: each chunk keeps the lane -> trajectory pairs it was launched with) and is
    re-admitted one chunk later.  Trajectories are exact-seeded, so both give the same
    trajectories 1..n_i per worker with the same transitions."""
    c = eng.ctx
    L, S, A, K, dev = eng.B, c.S, c.A, eng.K, c.device
    R = eng.term.horizon
    adm = _Admission(W, quota, mode, base_seed, R, speculate, L, c.M, eng.member_blocks)
    store = _Store(dev, S, A, W * (quota + R) if mode == "samples" else W * quota * 64)
    ring = _ChunkRing(eng, K) if pipeline else None
    eng.eval_mode = eval_mode
    ref_noise = rng == "reference" and not eval_mode
    hn = _HostNoise(c.lib, L, K, A) if ref_noise else None
    noise_dev = _noise_buffer(eng, K, L, A) if ref_noise else None
    # pinned staging; pipelined two sets: set i % 2 is rewritten only after chunk i - 2 has completed
    rows_dtype = torch.float64 if eng.motion is not None else torch.int32
    stage = [_Stage(L, K, rows_dtype, dev, pipeline) for _ in range(2 if pipeline else 1)]
    reset_devs = (torch.empty(L, dtype=torch.uint8, device=dev), torch.empty(L, dtype=torch.int32, device=dev),
                  torch.empty(L, dtype=rows_dtype, device=dev))
    # (the DTW score needs every trajectory's reset time; the reference draw is the host's already)
    t_out = torch.empty(L, dtype=torch.float64, device=dev) if dtw is not None and rng != "reference" else None
    pre_drawn = False  # the lanes of the previous chunk already hold their next K draws
    chunk_graph = None
    chunks, budget = 0, 4 * (W * quota + W) * (R + K) // K + 64
    pending = None  # pipelined: (stage set, [(lane, trajectory)], lanes) of the queued, unread chunk

    def read_back(si: int, launched, lanes: np.ndarray) -> None:
        st = stage[si]
        if not pipeline:
            done = eng.done[:K].cpu().numpy()  # [K, L]: the chunk's one host sync
        else:
            if st.event is not None:
                st.event.synchronize()
            done = st.done.numpy()
        live = adm.live(launched)
        if not live:
            return
        if len(live) < len(launched):
            lanes = np.array([b for b, _ in live], np.int64)
        n, hit, starts, flat = _chunk_rows(done.astype(bool)[:, lanes], lanes, L)
        # ---- compact the live lanes' transitions into the store ----
        if not pipeline:
            base = store.append_from(_chunk_arrays(eng, K), torch.from_numpy(flat).to(dev))
        else:
            # pinned + non_blocking: a pageable upload would wait for the chunk queued behind this one
            st.flat.numpy()[:flat.size] = flat
            idx = st.flat_dev[:flat.size]
            idx.copy_(st.flat[:flat.size], non_blocking=True)
            base = store.append_from(ring.slots[si], idx)
        adm.advance(live, n, hit, base + starts)

    while True:
        new = adm.admit()
        launched = adm.in_flight()
        # nothing to admit and every trajectory in flight reaches the horizon inside the queued
        # chunk (its length through the chunks read back + K >= R): another chunk would only step
        # idle lanes -- read the queued one back first
        tail = pending is not None and not new and all(tr.length + K >= R for _, tr in launched)
        if not launched or tail:
            if pending is None:
                break
            read_back(*pending)  # the last queued chunk may end trajectories or free admissions
            pending = None
            continue
        chunks += 1
        if chunks > budget:
            raise RuntimeError("sample_points: step budget exhausted (trajectories longer than the horizon?)")
        si = chunks % len(stage)
        st = stage[si]
        active = np.array([b for b, _ in launched], np.int64)
        new_lanes = np.array([tr.lane for tr in new], np.int64)
        _reset_lanes(eng, st, reset_devs, active, new, rng, time_max, t_out)
        # ---- K synchronous steps ----
        if hn is not None:
            hn.join()
            if new:
                hn.seed(new_lanes, np.array([tr.seed for tr in new]))  # np.random.seed (sampler.py:39)
            # the next K draws of every lane in flight (finished ones idle), the continuing lanes'
            # drawn ahead during the previous chunk
            buf = hn.draw(new_lanes if pre_drawn else active, hn.bufs[chunks % 3])
            noise_dev.copy_(buf, non_blocking=True)
        # (the first chunk of a new shape allocates the workspaces: captured from the second on)
        if graph and chunk_graph is None and (chunks >= 2 or "_chunk_graphs" in eng.__dict__):
            chunk_graph = _chunk_graph(eng, K, noise_dev, eval_mode)
        if chunk_graph is not None:
            chunk_graph.replay()
        else:
            for k in range(K):
                eng.step(noise=None if noise_dev is None else noise_dev[k])
        if pipeline:
            ring.snapshot(eng, si)
            st.done.copy_(eng.done[:K], non_blocking=True)
            if st.event is not None:
                st.event.record()
        if hn is not None:
            # the next chunk's draws of this chunk's lanes while the GPU steps (pipelined: on a host
            # thread while chunk c - 1 is read back; buffer (c + 1) % 3 last served chunk c - 2,
            # whose upload completed before it was read back); a lane that ends or is dropped is
            # re-seeded and re-drawn if admitted again, so its surplus draws are never used
            hn.draw_ahead(active, (chunks + 1) % 3, background=pipeline)
            pre_drawn = True
        if not pipeline:
            read_back(si, launched, active)
            continue
        if pending is not None:
            read_back(*pending)
        pending = (si, launched, active)
    if hn is not None:
        hn.join()
    # ---- reorder into path order on the device, one copy to the host ----
    trajs = adm.trajectories()
    if not trajs:
        return [], 0
    paths, n = _build_paths(trajs, store, eng, dev)
    if dtw is not None:
        _deliver_dtw(dtw, trajs, paths)
    return paths, n


def sample_points(env, policy, num_to_collect: int, base_seed: int = 0, num_workers: int = 4, mode: str = "samples",
                  eval_mode: bool = False, verbose: bool = False, deepmimic: bool = False, rng: str = "reference",
                  chunk: int = 16, speculate: bool = True, graph: bool = True, pipeline: bool = True,
                  member_blocked: bool = True, dtw=None):
    """milo.sampler.sample_points on the GPU.  `env` is a BatchedSimEnv (or a RolloutEngine):
    its ensemble, reset source, reset-time window (reset_args custom_time / time_max) and
    termination are used, and its lane count caps the concurrency; `policy` a DevicePolicy or
    the reference's mjrl MLP (wrapped and kept in sync by device_policy).  Returns the reference's list of path dicts
    (observations / next_observations / actions float64, rewards 0, agent_infos {mean,
    log_std, evaluation}, env_infos, terminated).  A missing info['valid'] counts as valid
    (SimEnv returns {}; the reference's deepmimic=True branch, sampler.py:61, would raise).
    `speculate`: admit beyond the worst-case reservation from the observed trajectory lengths
    (same result, see _Admission); `graph`: replay each chunk's steps as a captured HIP graph;
    `pipeline`: queue chunk i before reading chunk i-1's done flags (same result, see
    _collect); `member_blocked` (f16x3 ensembles with M >= 2): every lane steps through
    its trajectory's member only, as SimEnv.step does (the engine's lanes in M blocks of a
    multiple of 128; a quarter of the ensemble rows per step at M = 4), instead of all M members
    on every lane (same paths up to the GEMM's fp32 rounding).  `dtw` (a dtw.TimeWarper on the
    env's ReferenceMotion): every path also carries path['reset_time'] and
    env_infos[-1]['dtw_cost'], the evaluation's score as gym_deepmimic.py:160-162 delivers it;
    without it the dicts hold neither key."""
    assert mode == "samples" or mode == "trajectories"
    if rng not in ("reference", "device"):
        raise ValueError("rng must be 'reference' or 'device'")
    src = env.engine if isinstance(env, BatchedSimEnv) else env
    W = int(num_workers)
    quota = math.ceil(num_to_collect / W)  # sampler.py:113
    R = src.term.horizon
    need = W * (math.ceil(quota / R) if mode == "samples" else quota)
    if speculate and mode == "samples":
        need *= 4  # room for trajectories shorter than the horizon (lengths ~R/4) to run at once
    lanes = max(1, min(need, src.B))
    M = src.ctx.M
    Bq = 0
    if member_blocked and M >= 2 and src.ens.W2 is not None:
        # member blocks of a multiple of 128 lanes, rounded down: the lanes in flight at once stay
        # well below the speculative estimate (~125 of 544 at 40 000 samples), and a member's
        # single 128-row tile runs the 8-wave small-row GEMM (68 vs 85 us per forward at 256)
        Bq = max(128, math.ceil(need / M) // 128 * 128)
        while Bq > 128 and M * Bq > max(src.B, M * 128):
            Bq -= 128
        lanes = M * Bq
    K = max(1, min(int(chunk), R))
    time_max = _reset_time_max(env)
    if dtw is not None and src.motion is None:
        raise ValueError("sample_points: dtw needs a ReferenceMotion reset source (the score aligns with the clip)")
    policy = device_policy(env, policy)
    eng = _sampler_engine(env, lanes, K, policy, time_max, Bq)
    if rng == "device":
        policy.seed = (12345 + int(base_seed)) & 0xFFFFFFFFFFFFFFFF
    t0 = time.time()
    paths, n = (_collect(eng, W, quota, mode, int(base_seed), rng, eval_mode, time_max, speculate=speculate,
                         graph=graph, pipeline=pipeline, dtw=dtw)
                if quota > 0 else ([], 0))
    if verbose:
        print(f"Collected {n} and {len(paths)} trajectories in {time.time() - t0} seconds")
    return paths
