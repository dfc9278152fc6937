"""The host side of GAILCost.update_disc on the device (no GPU): the index draws
(costs.plan_disc_batch) and the replay ring's row mapping (datasets.ring_rows, AgentReplayBuffer
on the CPU) against fixture G16 (tests/golden/make_golden_dfit.py: the reference's own
update_disc), and the fp32 restatement tests/dfit_ref.py against G16's recorded run within a
quarter of the tolerances (TOL_DW = 2e-3, TOL_STATE = 3e-6: see test_gpu_dfit.py)."""
import os

import numpy as np
import pytest
import torch

import dfit_ref as R

G = R.G16
TOL_DW, TOL_STATE, TOL_METRIC = 2e-3, 3e-6, 1e-4


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g16_disc_update.npz"))


@pytest.mark.parametrize("name", list(G["blocks"]))
def test_plan_disc_batch_draws_as_the_reference(g16, name):
    from amp_extensions_amd.costs import plan_disc_batch
    cfg = G["blocks"][name]
    sample_rb = cfg["mb_seeds"] is None
    np.random.seed(cfg["seed"])   # the constructor's np.random.seed (gail_cost.py:63)
    for k in range(G["steps"]):
        idx_m, idx_e = plan_disc_batch(G["max_size"], G["n_expert"], cfg["bs"], sample_rb)
        assert np.array_equal(idx_e, g16[f"{name}_idx_e"][k])
        if sample_rb:
            assert np.array_equal(idx_m, g16[f"{name}_idx_m"][k])
        else:
            assert idx_m is None
    st = np.random.get_state()
    assert np.array_equal(np.concatenate([st[1], [st[2]]]).astype(np.int64), g16[f"{name}_rng_after"])


def test_ring_rows_match_concatenate_and_truncate():
    from amp_extensions_amd.datasets import AgentReplayBuffer, ring_rows
    _, adds, agent = R.g16_inputs()
    rb = AgentReplayBuffer(device="cpu", max_size=G["max_size"])
    assert len(rb) == 0 and rb.states is None
    want = None
    for s, s2 in adds:
        rb.add(s, s2)
        rows = torch.cat([s, s2], 1)
        want = (rows if want is None else torch.cat([want, rows], 0))[-G["max_size"]:]
        assert len(rb) == want.shape[0]
        assert torch.equal(torch.cat([rb.states, rb.next_states], -1), want)
        phys = ring_rows(rb.head, rb.n, rb.max_size, np.arange(rb.n))
        assert sorted(phys.tolist()) == list(range(rb.n)) and torch.equal(rb.ring[torch.from_numpy(phys)], want)
    assert rb.head != 0 and torch.equal(want, agent)        # the ring wrapped
    s, s2 = rb[5]
    assert torch.equal(torch.cat([s, s2]), want[5])
    np.random.seed(7)
    got = rb.sample(33)
    np.random.seed(7)
    assert torch.equal(got, want[np.random.randint(0, len(rb), 33)])
    with pytest.raises(IndexError):
        ring_rows(3, 10, 16, [10])
    # one add larger than the ring keeps its last max_size rows
    big = AgentReplayBuffer(device="cpu", max_size=50)
    big.add(*adds[0])
    assert torch.equal(torch.cat([big.states, big.next_states], -1), torch.cat(adds[0], 1)[-50:])


def test_empty_buffer_raises_as_the_reference():
    from amp_extensions_amd.datasets import AgentReplayBuffer
    rb = AgentReplayBuffer(device="cpu")
    with pytest.raises(Exception, match="Not possible to sample from empty dataset."):
        rb.sample(4)
    with pytest.raises(Exception, match="Not possible to select from empty dataset."):
        rb[0]


@pytest.mark.parametrize("name", list(G["blocks"]))
def test_fp32_restatement_reproduces_g16(g16, name):
    cfg = G["blocks"][name]
    expert, _, agent = R.g16_inputs()
    init = R.init_weights(2 * G["S"], G["hidden"], cfg["seed"])
    batches = [(expert[g16[f"{name}_idx_e"][k]],
                R.g16_mb(cfg, k) if cfg["mb_seeds"] else agent[g16[f"{name}_idx_m"][k]]) for k in range(G["steps"])]
    r = R.restate(init, batches, cfg["loss"], cfg["opt"], cfg["args"]["lr"], cfg["args"].get("momentum", 1e-8), 0.5,
                  0.05, 10.0, torch.float32)
    for k in range(G["steps"]):
        for j, key in enumerate(R.METRICS):
            ref = g16[f"{name}_metrics"][k][j]
            assert abs(r["metrics"][k][key] - ref) <= 0.25 * TOL_METRIC * abs(ref), (k, key)
    for j in range(6):
        e = R.update_error(r["weights"][j], g16[f"{name}_p{j}"], init[j])
        assert e <= 0.25 * TOL_DW, (R.NAMES[j], e)
        keys = [("buf", "s1")] if cfg["opt"] == "sgd" else [("exp_avg", "s1"), ("exp_avg_sq", "s2")]
        for fk, sk in keys:
            e = R.state_error(r["state"][sk][j], g16[f"{name}_p{j}_{fk}"])
            assert e <= 0.25 * TOL_STATE, (R.NAMES[j], fk, e)
    assert float(g16["tol_dw"]) == TOL_DW and float(g16["tol_state"]) == TOL_STATE
