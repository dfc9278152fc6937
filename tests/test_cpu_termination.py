"""The termination oracle (oracle.milo_ref.step_update_terminate) against G21: the reference's
own SimEnv.is_done (gym-simenv/gym_simenv/envs/sim_env.py:164-268), recorded by
tests/golden/make_golden_term.py over every state width, fall-body table and flag combination
of tests/term_cases.py.  `done`, `num_steps` and the velocity block that check_velocity rescales
in place are compared bit for bit; the GPU tests of the step kernels lean on both."""
import numpy as np
import pytest

import term_cases as T
from oracle import milo_ref as R

PAIRS = [(n, cfg) for n in T.CASE_NAMES for cfg in T.CASES[n]["configs"]]


@pytest.fixture(scope="module")
def g21(golden):
    return golden("g21_termination.npz")


def test_humanoid_table_is_the_oracles():
    assert tuple(R.FALL_BODIES) == T.HUMANOID_FALL and R.BODY_DEFS == T.HUMANOID_DEFS
    assert T.CASES["s197"]["vel_offset"] == 136 and T.CASES["s197"]["A"] == 36
    assert sorted((T.CASES[n]["S"] + 63) // 64 for n in T.CASE_NAMES) == list(range(1, 9))
    assert len(PAIRS) == 2 * 12 + 6 * 3 and len(T.FULL_CASES) == 2


@pytest.mark.parametrize("name,cfg", PAIRS)
def test_oracle_matches_reference_is_done(g21, name, cfg):
    c = T.load_case(name, g21)
    spec = c["spec"]
    vo = spec["vel_offset"]
    nxt, done, ns = R.step_update_terminate(c["ob"], c["pred"], c["num_steps"], **T.env_kwargs(spec, cfg))
    np.testing.assert_array_equal(done, g21[f"{name}__{cfg}__done"])
    np.testing.assert_array_equal(ns, c["num_steps"] + 1)
    plain = c["ob"] + c["pred"].astype(np.float64)
    np.testing.assert_array_equal(nxt[:, :vo], plain[:, :vo])
    f = T.config_flags(cfg)
    rescaled = f["enable_velocity_check"] and f["record_vel_as_pos"]
    np.testing.assert_array_equal(nxt[:, vo:], g21[f"{name}__vel"] if rescaled else plain[:, vo:])


def test_stored_conditions(g21):
    """The conditions the generator asserted on the inputs: both outcomes in every configuration,
    and every flag alone flips `done` on at least 8 rows of the humanoid case."""
    assert int(g21["horizon"]) == T.HORIZON
    for name, cfg in PAIRS:
        d = g21[f"{name}__{cfg}__done"]
        assert len(d) % 2 == 1 and 0 < d.sum() < len(d), (name, cfg)
    assert [str(x) for x in g21["flag_names"]] == [f[0] for f in T.FLAG_PAIRS]
    flips = [int((g21[f"s197__{a}__done"] != g21[f"s197__{b}__done"]).sum()) for _, a, b in T.FLAG_PAIRS]
    np.testing.assert_array_equal(g21["flip_counts"], flips)
    assert min(flips) >= T.MIN_FLIPS
