"""Inputs of the termination fixture G21 (tests/golden/g21_termination.npz), pure numpy.

Both tests/golden/make_golden_term.py (which runs the reference's SimEnv.is_done on these rows)
and the tests (which run the oracle and the HIP step kernels on them) build the rows from here;
the fixture stores a SHA-256 of every case's input arrays and `load_case` checks it, so an
input builder that drifts fails loudly instead of comparing against stale results.

A case is one state width S with one fall-body table; its rows are the same for every
configuration of the case.  Configurations are named "a{0,1}r{0,1}v{0,1,2}": record_all_world,
record_world_root_pos, and the velocity setting (0 check off, 1 check on, 2 check on with
record_vel_as_pos).  The layout follows gym-simenv/gym_simenv/envs/sim_env.py:101-104, 164-268:
body id i starts at (pos_dim + rot_dim) * i + 1, its y at +1, a capsule's normal y at
+pos_dim + 1; every listed body lies below vel_offset (the pose block precedes the velocities).

Rows (see `build_case`): every element of a row holds a distinct harmless value (bodies clear of
the ground under both root rules, |velocity| * 30 < 100, boxes *below* the ground since they
never collide), drawn from a pool of 7 base rows so that neighbouring lanes differ and neither
the 4-lane nor the 16-lane workgroups see a period.  On top of that:
  * fall rows: per listed sphere / capsule, per root rule (relative: root_y + rel_y, world), per
    capsule normal y in {0, 0.7, -1}: the checked expression one step below, on (where the
    threshold is reachable in fp64, else the first value above) and one step above the threshold.
    The relative-rule rows use a root y in [y/2, 2y] so that root_y + rel_y is exact (Sterbenz)
    and the threshold itself is reachable;
  * rule rows: a body at a fraction of its threshold with the root high: done only under the
    world rule of that list index (eight for list index 0, which record_world_root_pos governs);
  * velocity rows: elements vel_offset - 1 (never checked), vel_offset and S - 1 at |v| = 100 and
    one ulp either side, both signs, and the same around the v whose v / sampling_rate crosses 100;
    on the two checked elements also |v| = 50, 150 and 1000 (so that each velocity flag flips
    `done` on at least 8 rows);
  * horizon rows (num_steps + 1 == horizon, and one less), non-finite rows (NaN, +Inf, -Inf in a
    checked y, a checked velocity and an unchecked element) and a few plain rows.
The pinned elements are reached through the reference's own add ob + float64(pred): their pred
is a positive multiple of 2^-12, for which ob = want - pred is exact; the other preds are
arbitrary small float32 values, so the fp32 -> fp64 add matters everywhere.
"""
from __future__ import annotations

import hashlib
import json

import numpy as np

HORIZON = 9
SAMPLING_RATE = 1.0 / 30
VEL_THRESHOLD = 100.0  # check_velocity's default (sim_env.py:259)
POOL = 7

HUMANOID_FALL = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14)
HUMANOID_DEFS = {  # id: (shape, Param0, Param1); equal to oracle.milo_ref.BODY_DEFS (tested)
    0: ("sphere", 0.18, 0.18), 1: ("sphere", 0.22, 0.22), 2: ("sphere", 0.205, 0.205),
    3: ("capsule", 0.11, 0.3), 4: ("capsule", 0.1, 0.31), 5: ("box", 0.177, 0.055),
    6: ("capsule", 0.09, 0.18), 7: ("capsule", 0.08, 0.135), 8: ("sphere", 0.08, 0.08),
    9: ("capsule", 0.11, 0.3), 10: ("capsule", 0.1, 0.31), 11: ("box", 0.177, 0.055),
    12: ("capsule", 0.09, 0.18), 13: ("capsule", 0.08, 0.135), 14: ("sphere", 0.08, 0.08),
}

ALL_CONFIGS = tuple(f"a{a}r{r}v{v}" for a in (0, 1) for r in (0, 1) for v in (0, 1, 2))
# the default, all-world with the rescale, world-root-pos with the plain check
FEW_CONFIGS = ("a0r0v0", "a1r0v2", "a0r1v1")
# toggling each flag alone: (flag, configuration with it clear, configuration with it set)
FLAG_PAIRS = (("record_all_world", "a0r0v0", "a1r0v0"), ("record_world_root_pos", "a0r0v0", "a0r1v0"),
              ("enable_velocity_check", "a0r0v0", "a0r0v1"), ("record_vel_as_pos", "a0r0v1", "a0r0v2"))
MIN_FLIPS = 8


def config_flags(cfg: str) -> dict:
    a, r, v = int(cfg[1]), int(cfg[3]), int(cfg[5])
    return dict(record_all_world=bool(a), record_world_root_pos=bool(r), enable_velocity_check=v >= 1,
                record_vel_as_pos=v == 2)


def _synthetic_defs(ids, shapes, seed):
    rs = np.random.RandomState(seed)
    return {int(i): (s, round(float(rs.uniform(0.06, 0.25)), 3), round(float(rs.uniform(0.08, 0.35)), 3))
            for i, s in zip(ids, shapes)}


def _table32():
    ids = list(range(32))
    shapes = ["box" if i in (5, 11, 17) else ("capsule", "capsule", "sphere")[i % 3] for i in ids]
    return tuple(ids), _synthetic_defs(ids, shapes, 32)


def _case(S, A, fall, defs, vel_offset, configs, pos_dim=3, rot_dim=6, seed=0):
    return dict(S=S, A=A, fall_bodies=tuple(fall), body_defs=defs, vel_offset=vel_offset, configs=tuple(configs),
                pos_dim=pos_dim, rot_dim=rot_dim, seed=seed)


def _cases():
    c = {}
    # A checked element must lie below vel_offset, so a case either reaches the row's last slot with
    # a body (s100, s300, s512) or puts vel_offset on the last slot's boundary (s150, s350, s420).
    # NIT 1 (one slot: nothing to select): no bodies
    c["s40"] = _case(40, 4, (), {}, 30, FEW_CONFIGS, seed=40)
    # NIT 2: pos_dim / rot_dim 2 / 4 (stride 6); body 10 has y = 62 | normal y = 64, body 13 y = 80
    ids = (1, 3, 5, 8, 10, 13)
    c["s100"] = _case(100, 6, ids, _synthetic_defs(ids, ("capsule", "sphere", "box", "capsule", "capsule", "sphere"),
                                                   100), 85, FEW_CONFIGS, pos_dim=2, rot_dim=4, seed=100)
    # NIT 3: one body, not body 0 (y = 119, normal y = 122); first checked velocity at a slot boundary (128)
    c["s150"] = _case(150, 5, (13,), _synthetic_defs((13,), ("capsule",), 150), 128, FEW_CONFIGS, seed=150)
    # NIT 4: the humanoid
    c["s197"] = _case(197, 36, HUMANOID_FALL, dict(HUMANOID_DEFS), 136, ALL_CONFIGS, seed=197)
    # NIT 5: AMX_MAX_BODIES = 32 bodies, boxes inside; body 21 has y = 191 | normal y = 194 and
    # body 28 y = 254 | 257 on opposite sides of a slot boundary
    ids, defs = _table32()
    c["s300"] = _case(300, 8, ids, defs, 289, ALL_CONFIGS, seed=300)
    # NIT 6: the list starts at body 3 (body 0 comes third), a box inside; body 21 again; first
    # checked velocity just below a slot boundary (319 | 320)
    ids = (3, 21, 0, 12, 30, 34)
    c["s350"] = _case(350, 7, ids, _synthetic_defs(ids, ("capsule", "capsule", "sphere", "box", "sphere", "capsule"),
                                                   350), 319, FEW_CONFIGS, seed=350)
    # NIT 7: bodies in slots 1 to 5 (28: 254 | 257, 35: 317 | 320); first checked velocity just above a
    # slot boundary (384 | 385)
    ids = (41, 7, 28, 35, 14, 20)
    c["s420"] = _case(420, 9, ids, _synthetic_defs(ids, ("capsule", "sphere", "capsule", "capsule", "sphere",
                                                          "capsule"), 420), 385, FEW_CONFIGS, seed=420)
    # NIT 8: bodies in slots 0, 3 | 4 (254 | 257), 4 | 5 (317 | 320), 5, 6 and 7
    ids = (55, 49, 42, 35, 28, 0)
    c["s512"] = _case(512, 10, ids, _synthetic_defs(ids, ("capsule", "sphere", "capsule", "capsule", "capsule",
                                                          "sphere"), 512), 505, FEW_CONFIGS, seed=512)
    return c


CASES = _cases()
CASE_NAMES = tuple(CASES)
FULL_CASES = tuple(n for n in CASE_NAMES if CASES[n]["configs"] == ALL_CONFIGS)


def body_indexes(spec):
    """[(list index, shape, threshold, cylinder height, y index, normal-y index)] of the fall list."""
    out = []
    for li, bid in enumerate(spec["fall_bodies"]):
        shape, p0, p1 = spec["body_defs"][bid]
        off = (spec["pos_dim"] + spec["rot_dim"]) * bid + 1  # sim_env.py:103-104
        out.append((li, shape, 0.5 * p0 + 0.0001, p1, off + 1, off + spec["pos_dim"] + 1))  # :182, :189, :213
    return out


def _first(pred, lo=1e-9, hi=1e4):
    """Smallest positive double in [lo, hi] with pred true (pred monotone): bisection on the bit patterns."""
    a, b = np.float64(lo).view(np.int64), np.float64(hi).view(np.int64)
    assert not pred(np.float64(lo)) and pred(np.float64(hi))
    while b - a > 1:
        m = a + (b - a) // 2
        if pred(np.int64(m).view(np.float64)):
            b = m
        else:
            a = m
    return np.int64(b).view(np.float64)


def _straddle(f, thr):
    """(below, on, above) arguments of the monotone f around f(x) == thr; `on` is exact when reachable."""
    ge = _first(lambda x: f(x) >= thr)
    gt = _first(lambda x: f(x) > thr)
    return np.nextafter(ge, -np.inf), ge, gt


def _capsule_low(h, ny):
    """The lower of the two cap centres' offsets as check_capsule forms them (sim_env.py:213-236)."""
    top = 0.5 * h * ny
    bot = -0.5 * h * ny
    return lambda y: min(np.float64(y) + top, np.float64(y) + bot)


class _Rows:
    def __init__(self, spec):
        self.spec = spec
        S = spec["S"]
        rs = self.rs = np.random.RandomState(spec["seed"])
        self.bodies = body_indexes(spec)
        vo = spec["vel_offset"]
        self.checked = {0} | {b[4] for b in self.bodies if b[1] != "box"} | {b[5] for b in self.bodies
                                                                              if b[1] == "capsule"}
        assert all(max(b[4], b[5]) < vo for b in self.bodies) and 1 < vo < S
        assert (vo - 1) not in self.checked
        ob = 0.1 + 0.0007 * np.arange(S) + rs.uniform(0, 0.0005, (POOL, S))
        ob[:, vo:] *= np.where(np.arange(S - vo) % 2 == 0, 1.0, -1.0)
        ob[:, 0] = 0.9 + rs.uniform(0, 0.01, POOL)
        for li, shape, thr, h, yi, nyi in self.bodies:
            ob[:, yi] = ob[:, yi] + 1.0 if shape != "box" else -0.5 - ob[:, yi]
        self.pool_ob = ob
        self.pool_pred = (rs.choice([-1.0, 1.0], (POOL, S)) * rs.uniform(0.001, 0.01, (POOL, S))).astype(np.float32)
        self.ob, self.pred, self.ns, self.kind = [], [], [], []

    def new(self, kind, ns=None):
        k = len(self.ob) % POOL
        self.ob.append(self.pool_ob[k].copy())
        self.pred.append(self.pool_pred[k].copy())
        self.ns.append(int(self.rs.randint(0, HORIZON - 2)) if ns is None else ns)
        self.kind.append(kind)
        return len(self.ob) - 1

    def pin(self, b, j, want):
        """ob'[j] = ob[j] + float64(pred[j]) becomes exactly `want`."""
        p = np.float32(int(self.rs.randint(5, 41)) * 2.0 ** -12)
        o = np.float64(want) - np.float64(p)
        for _ in range(8):
            s = o + np.float64(p)
            if s == want:
                break
            o = np.nextafter(o, np.inf if s < want else -np.inf)
        assert o + np.float64(p) == want, (j, want)
        self.ob[b][j], self.pred[b][j] = o, p


def build_case(name: str) -> dict:
    """ob [B, S] f64, pred [B, S] f32, num_steps [B] i32 of a case, with its spec, per-row kinds and digest."""
    spec = CASES[name]
    S, vo = spec["S"], spec["vel_offset"]
    R = _Rows(spec)
    exact = 0
    for li, shape, thr, h, yi, nyi in R.bodies:
        if shape == "box":
            continue
        for nyv in ((0.0, 0.7, -1.0) if shape == "capsule" else (None,)):
            f = (lambda y: np.float64(y)) if nyv is None else _capsule_low(h, nyv)
            tri = _straddle(f, thr)
            exact += int(f(tri[1]) == thr)
            for rule in ("rel", "world"):
                for yw in tri:
                    b = R.new(f"fall{li}")
                    if nyv is not None:
                        R.pin(b, nyi, nyv)
                    if rule == "world":
                        R.pin(b, yi, yw)
                    else:
                        r = np.float64(0.625) * tri[1] + np.float64(2.0 ** -20)
                        assert yw / 2 <= r <= 2 * yw and r + (yw - r) == yw
                        R.pin(b, 0, r)
                        R.pin(b, yi, yw - r)
        for c in (np.linspace(0.15, 0.85, 8) if li == 0 else (0.5,)):
            R.pin(R.new(f"rule{li}"), yi, np.float64(c) * thr)
    elems = (vo - 1, vo, S - 1)
    at = np.float64(VEL_THRESHOLD)
    plain = (np.nextafter(at, 0.0), at, np.nextafter(at, np.inf))
    scaled = _straddle(lambda v: np.float64(v) / SAMPLING_RATE, at)
    for j in elems:
        for sign in (1.0, -1.0):
            # (away from the thresholds too, on the checked elements: between the two, and beyond both)
            for v in plain + scaled + ((50.0, 150.0, 1000.0) if j >= vo else ()):
                R.pin(R.new("vel"), j, sign * np.float64(v))
    R.new("horizon", ns=HORIZON - 1)
    R.new("horizon", ns=HORIZON - 2)
    targets = [vo, vo - 1] + [b[4] for b in R.bodies if b[1] != "box"][:1]
    for j in targets:
        for val in (np.nan, np.inf, -np.inf):
            R.ob[R.new("nonfinite")][j] = val
    for _ in range(5 + len(R.ob) % 2):  # a few plain rows; an odd row count
        R.new("plain")
    ob, pred, ns = np.array(R.ob, np.float64), np.array(R.pred, np.float32), np.array(R.ns, np.int32)
    assert ob.shape[0] % 2 == 1 and ob.shape == pred.shape == (len(ns), S)
    fin = np.isfinite(ob)
    nxt = np.where(fin, ob, 0.0) + pred.astype(np.float64)
    assert all(len(np.unique(r)) == S for r in nxt)  # distinct within every row
    return dict(name=name, spec=spec, ob=ob, pred=pred, num_steps=ns, kinds=tuple(R.kind), exact_on_rows=exact,
                sha=digest(spec, ob, pred, ns))


def digest(spec, ob, pred, ns) -> str:
    h = hashlib.sha256()
    h.update(json.dumps({k: (sorted((int(i), list(d)) for i, d in v.items()) if k == "body_defs" else v)
                         for k, v in spec.items()}, sort_keys=True).encode())
    for a in (ob, pred, ns):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


_CACHE = {}


def load_case(name: str, fixture) -> dict:
    """build_case(name), checked against the digest stored in the loaded fixture; cached and read-only."""
    if name not in _CACHE:
        c = build_case(name)
        assert c["sha"] == str(fixture[f"{name}__sha"]), f"term_cases.{name}: the inputs no longer match G21's digest"
        for k in ("ob", "pred", "num_steps"):
            c[k].setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def env_kwargs(spec, cfg: str) -> dict:
    """Keyword arguments of oracle.milo_ref.SimEnvRef / step_update_terminate for (case, configuration)."""
    return dict(horizon=HORIZON, sampling_rate=SAMPLING_RATE, vel_offset=spec["vel_offset"],
                fall_bodies=list(spec["fall_bodies"]), body_defs=spec["body_defs"], pos_dim=spec["pos_dim"],
                rot_dim=spec["rot_dim"], **config_flags(cfg))
