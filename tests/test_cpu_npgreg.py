"""CPU-only checks of the NPG planner's BC term and subsampled Fisher: the fp32 comparator
tests/npgreg_ref.py reproduces G23's recorded reference run (two consecutive
NPG.train_from_paths calls with hvp_sample_frac 0.5 and bc_args) within the project's NPG bounds
and re-draws its index vectors; the conditions that keep the GPU tests honest hold for G23 and
for every oracle-shape case (the BC gradient matters, subsampling matters, the fp32 comparator
sits well inside every bound of its fp64 restatement); the new entry points are bound, declared
and exported, and refuse bad arguments before anything touches a GPU."""
import ctypes

import numpy as np
import pytest

import npgreg_ref as G
from amp_extensions_amd import _build, _native

S23, A23 = 226, 28
NEW = ("amx_npg_pass_idx", "amx_npg_pass_cg_idx", "amx_npg_ll", "amx_npg_ll_blocks")


@pytest.fixture(scope="module")
def lib():
    return _native.load(_build.build(verbose=False))


@pytest.fixture(scope="module")
def g23(golden):
    g = golden("g23_npg_reg.npz")
    bc = (g["expert_obs"].astype(np.float64), g["expert_act"], float(g["reg_coeff"]))
    calls, params = [], g["params0"]
    for k in range(2):
        c = {key: g[f"c{k}__{key}"] for key in ("observations", "actions", "adv_whitened", "idx", "vpg", "npg",
                                                 "params", "surr_before", "surr_after")}
        c["params_in"] = params
        args = (params, S23, A23, c["observations"].astype(np.float64), c["actions"], c["adv_whitened"])
        c["ref"] = G.update(*args, idx=list(c["idx"]), bc=bc)
        c["ref64"] = G.update64(*args, idx=list(c["idx"]), bc=bc)
        c["full"] = G.update(*args, idx=None, bc=bc)
        c["other"] = G.update(*args, idx=G.draws(int(g["numpy_seed"]) + 1 + k, len(c["actions"]), float(g["frac"])),
                              bc=bc)
        calls.append(c)
        params = c["params"]
    return g, calls


def test_comparator_reproduces_g23(g23):
    g, calls = g23
    for c in calls:
        r, p0 = c["ref"], c["params_in"]
        assert r["products"] == int(g["cg_iters"])
        assert G.maxrel(r["vpg"], c["vpg"]) <= G.TOL_VPG
        assert G.maxrel(r["npg"], c["npg"]) <= G.TOL_NPG
        assert G.maxrel(r["params1"].astype(np.float64) - p0, c["params"].astype(np.float64) - p0) <= G.TOL_NPG
        np.testing.assert_allclose(r["surr_after"], float(c["surr_after"]), rtol=G.RTOL_SURR)
        assert abs(r["surr_before"] - float(c["surr_before"])) <= G.ATOL_SURR_BEFORE


def test_index_draws_from_the_recorded_seed(g23):
    g, calls = g23
    rs = np.random.RandomState(int(g["numpy_seed"]))
    for c in calls:
        n = len(c["actions"])
        idx = np.asarray(G.draws(rs, n, float(g["frac"]), int(g["cg_iters"])))
        assert idx.shape == c["idx"].shape == (10, int(float(g["frac"]) * n))
        assert np.array_equal(idx, c["idx"])
    st = rs.get_state()
    assert np.array_equal(st[1], g["rng_keys"]) and st[2] == int(g["rng_pos"])


def conditions(ref, ref64, full, other, p0, with_bc):
    """The conditions that keep the GPU tests honest, on the comparator."""
    if with_bc:  # the BC term matters: a dropped or mis-scaled term breaks the 1e-4 VPG check
        ratio = np.linalg.norm(ref["vpg_bc"]) / np.linalg.norm(ref["vpg_rollout"])
        assert 0.1 <= ratio <= 10.0, ratio
    # subsampling matters: the full Fisher, or another seed's rows, miss the 2e-3 bound tenfold
    assert G.maxrel(full["npg"], ref["npg"]) > 10 * G.TOL_NPG
    assert G.maxrel(other["npg"], ref["npg"]) > 10 * G.TOL_NPG
    # the fp32 comparator sits within a quarter of every bound of its fp64 restatement
    dp = ref["params1"].astype(np.float64) - p0
    assert G.maxrel(ref["vpg"], ref64["vpg"]) <= G.TOL_VPG / 4
    assert G.maxrel(ref["npg"], ref64["npg"]) <= G.TOL_NPG / 4
    assert G.maxrel(dp, ref64["params1_64"] - p0) <= G.TOL_NPG / 4
    assert abs(ref["surr_after"] / ref64["surr_after"] - 1) <= G.RTOL_SURR / 4
    assert abs(ref["surr_before"] - ref64["surr_before"]) <= G.ATOL_SURR_BEFORE / 4


def test_conditions_hold_for_g23(g23):
    _, calls = g23
    for c in calls:
        conditions(c["ref"], c["ref64"], c["full"], c["other"], c["params_in"], True)


@pytest.mark.parametrize("S,A,n,frac,with_bc", G.CASES)
def test_conditions_hold_for_oracle_cases(S, A, n, frac, with_bc):
    ref, ref64 = G.case_ref(S, A, n, frac, with_bc), G.case_ref(S, A, n, frac, with_bc, f64=True)
    full, other = G.case_ref(S, A, n, None, with_bc), G.case_ref(S, A, n, frac, with_bc, seed=G.DRAW_SEED + 1)
    assert ref["products"] == G.CG_ITERS and len(ref["idx"][0]) == int(frac * n)
    conditions(ref, ref64, full, other, G.case_inputs(S, A, n)["p0"], with_bc)


def test_new_symbols_bound_declared_and_exported(lib):
    declared = _native.header_symbols()
    for name in NEW:
        assert name in _native.SIGNATURES and name in declared
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert lib.amx_abi_version() == _native.ABI_VERSION == 2


def fake_ctx(S=197, A=36):
    """A zeroed amx_ctx stand-in with S and A set (device, n_cus, S, A lead the struct): every
    call below is refused before anything else of it is read."""
    buf = (ctypes.c_int * 512)()
    buf[2], buf[3] = S, A
    return buf, ctypes.cast(buf, ctypes.c_void_p)


D = ctypes.c_void_p(4096)  # a non-null dummy: the argument checks never dereference it


def refused(lib, rc, *words):
    assert rc == -1
    msg = lib.amx_last_error()
    assert all(w in msg for w in words), msg


def test_indexed_pass_and_ll_refuse_bad_arguments(lib):
    _keep, ctx = fake_ctx()

    def pidx(ctx_=ctx, N=64, M=32, idx=D, dtype=_native.AMX_IN_F32, rpb=32, vec=D):
        return lib.amx_npg_pass_idx(ctx_, N, M, idx, D, dtype, 197, D, vec, rpb, D, None, None, None, None)

    refused(lib, pidx(ctx_=None), b"amx_npg_pass_idx", b"null ctx")
    refused(lib, pidx(M=0), b"amx_npg_pass_idx", b"M=0")
    refused(lib, pidx(idx=None), b"amx_npg_pass_idx", b"null buffer")
    refused(lib, pidx(dtype=_native.AMX_IN_F64), b"amx_npg_pass_idx", b"fp32 observations")
    refused(lib, pidx(rpb=48), b"amx_npg_pass_idx", b"rows_per_block=48")
    refused(lib, pidx(vec=None), b"amx_npg_pass_idx", b"vec")

    def pcg(M=32, dtype=_native.AMX_IN_F32, r_out=ctypes.c_void_p(8192)):
        return lib.amx_npg_pass_cg_idx(ctx, 64, M, D, D, dtype, 197, D, 32, D, None, 0.0, D, D, r_out,
                                       D, ctypes.c_void_p(8192), D, D, ctypes.c_void_p(8192), D, None, None)

    refused(lib, pcg(M=0), b"amx_npg_pass_cg_idx", b"M=0")
    refused(lib, pcg(dtype=_native.AMX_IN_F64), b"amx_npg_pass_cg_idx", b"fp32 observations")
    refused(lib, pcg(r_out=D), b"amx_npg_pass_cg_idx", b"alternate buffers")

    refused(lib, lib.amx_npg_ll(None, 64, D, 197, D, 36, D, D, None, None, None), b"amx_npg_ll", b"null ctx")
    refused(lib, lib.amx_npg_ll(ctx, 0, D, 197, D, 36, D, D, None, None, None), b"amx_npg_ll", b"N=0")
    refused(lib, lib.amx_npg_ll(ctx, 64, D, 197, D, 36, D, None, None, None, None), b"amx_npg_ll", b"partials")
    assert lib.amx_npg_ll_blocks(None, 64) == -1 and lib.amx_npg_ll_blocks(ctx, 0) == -1
    assert lib.amx_npg_ll_blocks(ctx, 65) == 1  # n_cus 0 in the stand-in: one workgroup


class _Lin:
    def __init__(self, o, i):
        import torch
        self.weight, self.bias = torch.zeros(o, i), torch.zeros(o)


class _Model:
    def __init__(self, sizes, transformations=None):
        self.fc_layers = [_Lin(sizes[k + 1], sizes[k]) for k in range(len(sizes) - 1)]
        if transformations is not None:
            self.transformations = transformations


class _Pol:
    def __init__(self, sizes, transformations=None):
        self.model = _Model(sizes, transformations)


def test_drop_in_refusals_need_no_gpu():
    from amp_extensions_amd.npg import NPG
    with pytest.raises(NotImplementedError, match="input normalization"):
        NPG(None, _Pol((11, 32, 32, 3)), None, input_normalization=0.5)
    with pytest.raises(NotImplementedError, match="transformations"):
        NPG(None, _Pol((11, 32, 32, 3), dict(in_shift=np.zeros(11), in_scale=None, out_shift=None, out_scale=None)),
            None)
    with pytest.raises(NotImplementedError, match="hidden sizes"):
        NPG(None, _Pol((11, 64, 64, 3)), None)
    # the reference ignores an input_normalization outside (0, 1] (npg_cg.py:61-63); so does the drop-in
    agent = NPG(None, _Pol((11, 32, 32, 3)), None, input_normalization=1.5, kl_dist=0.05, hvp_sample_frac=0.5,
                FIM_invert_args={"iters": 10, "damping": 1e-4})
    assert agent.input_normalization is None and agent.n_step_size == 0.1 and agent.hvp_subsample == 0.5
    assert agent.alpha is None and agent.running_score is None and agent.bc_args["flag"] is False
    assert agent.FIM_invert_args == {"iters": 10, "damping": 1e-4} and hasattr(agent.logger, "log_kv")
