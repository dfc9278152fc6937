"""Generate tests/golden/g21_termination.npz by running the REFERENCE SimEnv.is_done.

Dev-container only, like make_golden.py (whose stubs and paths it reuses): imports the
reference from $AMX_REFERENCE (make_golden.py's default) and exits cleanly when it is absent.
No reference source is copied; the fixture holds recorded results and digests only.

G21: for every case of tests/term_cases.py (one state width S = 40 ... 512 with one fall-body
table) and every configuration of the case (record_all_world x record_world_root_pos x velocity
check off / on / on with record_vel_as_pos), a SimEnv built by object.__new__ with the attributes
is_done, check_sphere, check_capsule, check_collision and check_velocity read
(gym-simenv/gym_simenv/envs/sim_env.py:164-268) runs, per row,
    env.ob = ob + pred.astype(np.float32)   (the add of sim_env.py:158)
    env.num_steps = num_steps + 1           (:153)
    done = env.is_done()
and the fixture records `done` and, where the check rescales in place (:264-267), the velocity
block of the mutated env.ob (identical for every such configuration of a case: asserted, stored
once).  The inputs are rebuilt from seeds by tests/term_cases.py; their SHA-256 is stored.

Asserted here and stored: in every configuration 0 < done.sum() < rows; for each of the four
flags at least 8 rows of the humanoid case change `done` when that flag alone is toggled
(term_cases.FLAG_PAIRS; `flip_counts`).  The file is written with fixed zip timestamps, so a
rerun is byte-identical.

    python tests/golden/make_golden_term.py
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, REF, install_stubs  # noqa: E402
import term_cases as T  # noqa: E402


class VelOffsetCore:
    """Stands in for DeepMimicEnv in check_velocity (sim_env.py:263)."""

    def __init__(self, vel_offset):
        self.vel_offset = vel_offset

    def get_vel_offset(self):
        return self.vel_offset


def make_env(SimEnv, spec, cfg):
    env = object.__new__(SimEnv)
    for k, v in T.config_flags(cfg).items():
        setattr(env, k, v)
    env.horizon = T.HORIZON
    env.sampling_rate = T.SAMPLING_RATE
    env.deepmimic = VelOffsetCore(spec["vel_offset"])
    env.pos_dim, env.rot_dim = spec["pos_dim"], spec["rot_dim"]
    env.fall_contact_bodies = np.array(spec["fall_bodies"], dtype=np.int64)
    env.fall_contact_bodies_offset = (env.pos_dim + env.rot_dim) * env.fall_contact_bodies + 1
    env.fall_contact_bodies_params = [[spec["body_defs"][i][1], spec["body_defs"][i][2], 0.0]
                                      for i in spec["fall_bodies"]]
    env.fall_contact_bodies_shapes = [spec["body_defs"][i][0] for i in spec["fall_bodies"]]
    return env


def write_npz(path, arrays):
    """np.savez_compressed with sorted members and a fixed timestamp (byte-identical reruns)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if not os.path.isdir(os.path.join(REF, "gym-simenv")):
        print(f"{REF} is absent: nothing generated")
        return 0
    install_stubs()
    from gym_simenv.envs.sim_env import SimEnv

    out = {"horizon": np.int64(T.HORIZON), "flag_names": np.array([f[0] for f in T.FLAG_PAIRS])}
    done_of = {}
    for name in T.CASE_NAMES:
        c = T.build_case(name)
        spec, vo = c["spec"], c["spec"]["vel_offset"]
        B = c["ob"].shape[0]
        out[f"{name}__sha"] = np.array(c["sha"])
        vel = None
        for cfg in spec["configs"]:
            env = make_env(SimEnv, spec, cfg)
            done = np.zeros(B, np.uint8)
            blocks = np.zeros((B, spec["S"] - vo))
            for b in range(B):
                env.ob = c["ob"][b] + c["pred"][b].astype(np.float32)
                env.num_steps = int(c["num_steps"][b]) + 1
                done[b] = bool(env.is_done())
                blocks[b] = env.ob[vo:]
            assert 0 < done.sum() < B, (name, cfg, int(done.sum()), B)
            out[f"{name}__{cfg}__done"] = done
            done_of[name, cfg] = done
            if env.enable_velocity_check and env.record_vel_as_pos:
                assert vel is None or np.array_equal(vel, blocks, equal_nan=True)
                vel = blocks
        out[f"{name}__vel"] = vel
        print(f"{name}: rows {B}, exact on-threshold rows {c['exact_on_rows']}, done per configuration",
              {cfg: int(done_of[name, cfg].sum()) for cfg in spec["configs"]})
    flips = np.array([int((done_of["s197", a] != done_of["s197", b]).sum()) for _, a, b in T.FLAG_PAIRS], np.int64)
    print("flip_counts", dict(zip([f[0] for f in T.FLAG_PAIRS], flips.tolist())))
    assert (flips >= T.MIN_FLIPS).all(), flips
    out["flip_counts"] = flips
    path = os.path.join(OUT, "g21_termination.npz")
    write_npz(path, out)
    print("wrote g21_termination.npz", os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
