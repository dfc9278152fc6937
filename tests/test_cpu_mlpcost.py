"""MLPCost's host half without a GPU: the seeded net and bandwidth against the reference's own
records (G22, tests/golden/make_golden_mlpcost.py), the fp64 restatement (tests/mlpcost_ref.py)
against the reference's fp32 records, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpcost_ref as R  # noqa: E402

from amp_extensions_amd import _build  # noqa: E402
from amp_extensions_amd.costs import check_mlp_cost_config, fit_bandwidth, mlp_cost_net  # noqa: E402

VARIANTS = sorted(R.G22)


def g22_inputs(name):
    cfg, C = R.G22[name], R.G22_COMMON
    es, ea, es2 = R.synthetic_rows(C["n_expert"], C["expert_seed"], cfg["S"], cfg["A"])
    ps, pa, ps2 = R.synthetic_rows(C["n_pi"], C["pi_seed"], cfg["S"], cfg["A"], shift=C["pi_shift"])
    return cfg, C, R.cost_rows(cfg["input_type"], es, ea, es2), R.cost_rows(cfg["input_type"], ps, pa, ps2), (ps, pa, ps2)


def g22_state_dict(g, name):
    pre = f"{name}__sd__"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("name", VARIANTS)
def test_seeded_net_and_bandwidth_are_the_references(golden, name):
    """mlp_cost_net under the reference's seeding order (torch, numpy, the Linear layers, then the
    bandwidth draw) reproduces G22's state_dict bit for bit, with its keys, and its bw with ==."""
    g = golden("g22_mlp_cost.npz")
    cfg, C, expert, _, _ = g22_inputs(name)
    torch.manual_seed(C["seed"])
    np.random.seed(C["seed"])
    net = mlp_cost_net(expert.shape[1], cfg["hidden_dims"], cfg["feature_dim"])
    bw = fit_bandwidth(expert, C["bw_samples"], C["bw_quantile"])
    want = g22_state_dict(g, name)
    sd = net.state_dict()
    assert list(sd) == sorted(want, key=lambda k: (int(k.split(".")[0]), k.split(".")[1] == "bias"))
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), want[k]), k
    assert bw == float(g[f"{name}__bw"])
    assert isinstance(net[len(net) - 1], torch.nn.Tanh)
    n_hidden = len(cfg["hidden_dims"])
    assert sum(isinstance(m, torch.nn.Linear) for m in net) == (n_hidden + 1 if n_hidden > 1 else 1)


@pytest.mark.parametrize("name", VARIANTS)
def test_fp64_restatement_agrees_with_the_references_fp32_records(golden, name):
    """The reference's recorded fp32 results lie within the yardstick error of the fp64
    restatement: per element twice the error of this machine's own torch fp32 evaluation (another
    torch build may sum in another order), the scalars within the bounds propagated from that."""
    g = golden("g22_mlp_cost.npz")
    cfg, C, expert, x_pi, (ps, pa, ps2) = g22_inputs(name)
    rec = lambda k: np.asarray(g[f"{name}__{k}"], np.float64)
    ref = R.Ref64(g22_state_dict(g, name), expert, cfg["feature_dim"], cfg["cost_range"], C["lambda_b"])
    mmd = ref.fit_cost(x_pi)
    y = R.Yardstick(ref, expert, x_pi)
    d_phi, d_w, d_phi_e = 2 * y.phi_err, 2 * y.w_err, 2 * y.phi_e_err
    phi = ref.rep(x_pi)
    assert np.abs(rec("phi_pi") - phi[::R.G22_PHI_STRIDE]).max() <= d_phi
    assert np.abs(rec("phi_e") - ref.phi_e).max() <= d_phi_e
    assert np.abs(rec("w") - ref.w).max() <= d_w
    assert abs(float(rec("mb_mmd")) - mmd) <= R.mmd_bound(ref.w, d_w)
    row = R.dot_bound(phi, ref.w, d_phi, d_w)
    assert (np.abs(rec("costs")[:, 0] - ref.get_costs(x_pi)) <= row).all()
    assert (np.abs(rec("v_targ")[:, 0] - ref.get_costs(x_pi)) <= row).all()
    lam = C["lambda_b"]
    # the recorded weighted bonus is the reference ensemble's: taken as given
    wb = rec("bonus")[:, 0]
    ipm = (1 - lam) * ref.get_costs(x_pi)
    slack = R.ulp4(ipm, wb)
    assert (np.abs(rec("ipm")[:, 0] - ipm) <= (1 - lam) * row + slack).all()
    assert (np.abs(rec("cost")[:, 0] - (ipm - wb)) <= (1 - lam) * row + slack).all()
    if cfg["cost_range"] is not None:
        erow = R.dot_bound(ref.expert_rep, ref.w, d_phi, d_w)
        assert abs(float(rec("expert_cost")) - ref.expert_cost()) <= (1 - lam) * erow.mean() + R.ulp4(ref.expert_cost())
    else:
        assert f"{name}__expert_cost" not in g.files


def test_unsupported_configurations_are_refused():
    with pytest.raises(NotImplementedError, match="relu"):
        check_mlp_cost_config([64, 64], "tanh", 128)
    # one hidden width other than feature_dim: the reference emits features of that width but
    # scales by feature_dim; the message names the quirk
    with pytest.raises(NotImplementedError, match=r"width 64 yet scales them by\s+sqrt\(2 / 128\)"):
        check_mlp_cost_config([64], "relu", 128)
    with pytest.raises(ValueError, match="multiple of 128"):
        check_mlp_cost_config([64, 64], "relu", 100)
    for hidden in ([], [128], [64, 96, 64], [512] * 4):
        check_mlp_cost_config(hidden, "relu", 128)
    # [F] alone is the flat net at width F
    torch.manual_seed(0)
    net = mlp_cost_net(10, [128], 128)
    assert [type(m).__name__ for m in net] == ["Linear", "Tanh"] and net[0].out_features == 128


def test_constructor_refuses_before_anything_is_uploaded():
    """The refusals come first in MLPCost.__init__: they raise on a machine without a GPU, where
    creating a context or uploading anything would fail differently."""
    from amp_extensions_amd.costs import MLPCost
    expert = torch.zeros(8, 10)
    with pytest.raises(NotImplementedError):
        MLPCost(expert, hidden_dims=[64, 64], activation="tanh", feature_dim=128, device="cpu")
    with pytest.raises(NotImplementedError):
        MLPCost(expert, hidden_dims=[64], feature_dim=128, device="cpu")
    with pytest.raises(ValueError):
        MLPCost(expert, hidden_dims=[64, 64], feature_dim=100, device="cpu")
    with pytest.raises(NotImplementedError):
        MLPCost(expert, hidden_dims=[64, 64], feature_dim=128, input_type="xyz", device="cpu")
    with pytest.raises(TypeError):  # any gemm other than f16x3 is not offered
        MLPCost(expert, hidden_dims=[64, 64], feature_dim=128, gemm="f32", device="cpu")


def test_package_exports_mlpcost_and_still_does_not_import_oracle():
    import amp_extensions_amd as amx
    from amp_extensions_amd.costs import MLPCost, RBFLinearCost
    assert amx.MLPCost is MLPCost and issubclass(MLPCost, RBFLinearCost) and "MLPCost" in amx.__all__
    for dp, _, fs in os.walk(_build.PKG_DIR):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_abi_additions_only():
    """amx_mlp_features_h3 is declared with amx_rff_features_h3's argument list and the ABI
    version is unchanged."""
    from amp_extensions_amd import _native as N
    assert N.SIGNATURES["amx_mlp_features_h3"] == N.SIGNATURES["amx_rff_features_h3"]
    assert "amx_mlp_features_h3" in N.header_symbols() and N.ABI_VERSION == 2
