"""Plain (dense_connect=False) dynamics ensembles, host side: the layer shapes, the padded
windowed parameter layout, the factory's dispatch and the refusals, and tests/plain_ref.py (the
comparator of test_gpu_plain.py) against the reference's own BasicMLP / DynamicsModel.train_step
run in fp64 (G24, tests/golden/make_golden_plain.py)."""
import numpy as np
import pytest
import torch

import plain_ref as PR

S, A = 197, 36


def _ckpt(golden_path, name="adam"):
    return torch.load(golden_path(f"g24_plain_{name}.pt"), map_location="cpu", weights_only=True)


@pytest.mark.parametrize("hidden", [[64], [64, 64], [64] * 3])
def test_layer_shapes(hidden):
    """(out, in) of BasicMLP(S + A, S, hidden, dense_connect=False) (dynamics.py:412-420): each
    layer's input is the previous layer's width alone."""
    from amp_extensions_amd.ensemble import BasicMLPWeights, basic_mlp_layer_shapes, plain_mlp_layer_shapes
    want = [(64, S + A)] + [(64, 64)] * (len(hidden) - 1) + [(S, 64)]
    assert plain_mlp_layer_shapes(S, A, hidden) == want == PR.plain_layer_shapes(S, A, hidden)
    net = BasicMLPWeights(S + A, S, hidden, dense_connect=False)
    assert [tuple(l.weight.shape) for l in net.fc_layers] == want and net.dense_connect is False
    assert list(net.state_dict()) == [f"fc_layers.{i}.{k}" for i in range(len(want)) for k in ("weight", "bias")]
    if len(hidden) > 1:  # the dense-connect shapes differ from the second layer on
        assert basic_mlp_layer_shapes(S, A, hidden)[1] == (64, S + A + 64)
    assert basic_mlp_layer_shapes(S, A, hidden)[0] == want[0]


def test_layer_shapes_are_the_reference_files(golden, golden_path):
    """The reference's own plain BasicMLP, as its save_ensemble wrote it."""
    from amp_extensions_amd.ensemble import plain_mlp_layer_shapes
    g = golden("g24_plain.npz")
    hidden = [int(x) for x in g["ck_hidden"]]
    for name in ("adam", "sgd"):
        sds = _ckpt(golden_path, name)
        assert len(sds) == 4
        for sd in sds:
            shapes = [tuple(sd["model"][f"fc_layers.{i}.weight"].shape) for i in range(len(hidden) + 1)]
            assert shapes == plain_mlp_layer_shapes(S, A, hidden)


@pytest.mark.parametrize("hidden", [[64], [64, 64], [64] * 3, [200, 200]])
def test_layout_round_trip(hidden):
    """state dict -> padded windowed layout -> state dict, bit for bit; pad rows and columns zero;
    W_0 [Hp][k0_pad], W_i [Hp][Hp], W_out [n_out_pad][Hp]."""
    from amp_extensions_amd.ensemble import init_model_weights
    from amp_extensions_amd.optstate import plain_ensemble_layout
    h, L = hidden[0], len(hidden)
    k0_pad, Hp, n_out_pad = 256, (h + 127) // 128 * 128, 256
    lay = plain_ensemble_layout(S, A, h, L, k0_pad, Hp, n_out_pad)
    assert lay.padded == [x for i in range(L + 1) for x in
                          (((n_out_pad if i == L else Hp), (k0_pad if i == 0 else Hp)), ((n_out_pad if i == L else Hp),))]
    assert lay.size == sum(int(np.prod(p)) for p in lay.padded)
    w = init_model_weights(S, A, hidden, 123, dense_connect=False)
    flat = [t for Wb in w for t in Wb]
    packed = lay.pack(flat)
    back = lay.unpack(packed)
    assert len(back) == len(flat)
    for x, y in zip(back, flat):
        assert x.shape == y.shape and torch.equal(x, y)
    mask = lay.live_mask()
    assert not packed[~mask].any() and int(mask.sum()) == sum(t.numel() for t in flat)
    for v, t in zip(lay.views(packed), flat):  # the live block is the leading one (no column remap)
        if t.dim() == 2:
            assert torch.equal(v[:t.shape[0], :t.shape[1]], t)
            assert not v[t.shape[0]:].any() and not v[:, t.shape[1]:].any()
        else:
            assert torch.equal(v[:t.shape[0]], t) and not v[t.shape[0]:].any()
    with pytest.raises(ValueError):  # a dense-connect member does not fit
        lay.pack([t for Wb in init_model_weights(S, A, hidden + [h], 1) for t in Wb][:len(flat)])


def test_factory_dispatches_on_dense_connect(monkeypatch):
    """dynamics_ensemble(...) takes the reference's arguments, defaults to plain (run.py's
    store_true flag) and returns the class dense_connect asks for."""
    from amp_extensions_amd import ensemble as E
    import amp_extensions_amd as amx
    assert amx.dynamics_ensemble is E.dynamics_ensemble and amx.PlainDynamicsEnsemble is E.PlainDynamicsEnsemble
    assert "dynamics_ensemble" in amx.__all__ and "PlainDynamicsEnsemble" in amx.__all__
    assert issubclass(E.PlainDynamicsEnsemble, E.DynamicsEnsemble)
    seen = []
    monkeypatch.setattr(E.DynamicsEnsemble, "_setup", lambda self, *a: seen.append(a))
    ds = object()
    e = E.dynamics_ensemble(S, A, ds, None, num_models=4, batch_size=256, hidden_sizes=[1024, 1024], transform=True,
                            optim_args={"optim": "adam", "lr": 1e-3, "eps": 1e-8}, base_seed=0,
                            device=torch.device("cpu"))
    assert type(e) is E.PlainDynamicsEnsemble and seen[-1][7] is False and seen[-1][6] == [1024, 1024]
    e = E.dynamics_ensemble(S, A, ds, None, dense_connect=False)
    assert type(e) is E.PlainDynamicsEnsemble
    e = E.dynamics_ensemble(S, A, ds, None, dense_connect=True, hidden_sizes=[512] * 4)
    assert type(e) is E.DynamicsEnsemble and seen[-1][7] is True
    e = E.dynamics_ensemble(S, A, ds, None, 4, 256, [64, 64], False, True)  # positional, as the reference's
    assert type(e) is E.DynamicsEnsemble and seen[-1][6] == [64, 64]


def test_refusals():
    from amp_extensions_amd.ensemble import DynamicsEnsemble, PlainDynamicsEnsemble, dynamics_ensemble
    ds = object()
    with pytest.raises(ValueError, match="DynamicsEnsemble"):
        PlainDynamicsEnsemble(S, A, ds, None, dense_connect=True)
    for cls in (PlainDynamicsEnsemble, dynamics_ensemble):
        for kw in (dict(use_resnet=True), dict(activation="tanh")):
            with pytest.raises(NotImplementedError):
                cls(S, A, ds, None, hidden_sizes=[64, 64], **kw)
    with pytest.raises(NotImplementedError) as e:  # the pinned raise, now naming where the feature lives
        DynamicsEnsemble(S, A, ds, None, hidden_sizes=[64, 64], dense_connect=False)
    assert "PlainDynamicsEnsemble" in str(e.value) and "dynamics_ensemble" in str(e.value)


def _rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def _norms(g):
    from amp_extensions_amd.datasets import AmpDataset
    from amp_extensions_amd.synthetic import offline
    tr = tuple(torch.from_numpy(x).float() for x in offline(int(g["n_offline"]), S, A, int(g["offline_seed"])))
    return tr, AmpDataset(*tr).get_transformations(torch.device("cpu"))


def test_fp64_restatement_matches_the_reference_forward(golden, golden_path):
    """plain_ref.forward in fp64 against the reference's BasicMLP(...).double() on the file's
    weights: fp64 rounding (different BLAS orders of a 233-term sum); the fp32 restatement
    against the reference's fp32 forwards: fp32 rounding."""
    g = golden("g24_plain.npz")
    sds = _ckpt(golden_path)
    _, norms = _norms(g)
    qs, qa = g["query_s"], g["query_a"]
    out = PR.forward(sds[0]["model"], norms, qs, qa, torch.float64)
    raw = PR.forward(sds[0]["model"], norms, qs, qa, torch.float64, unnormalize=False)
    assert _rel(out.numpy(), g["f64_preds"]) <= 1e-13 and _rel(raw.numpy(), g["f64_raw"]) <= 1e-13
    for k in range(4):
        p32 = PR.forward(sds[k]["model"], norms, qs, qa, torch.float32)
        assert _rel(p32.numpy(), g["preds"][k]) <= 2e-6
        assert _rel(PR.forward(sds[k]["model"], norms, qs, qa, torch.float64).numpy(), g["preds"][k]) <= 2e-5
    preds = torch.stack([PR.forward(sds[k]["model"], norms, qs, qa, torch.float64) for k in range(4)])
    np.testing.assert_allclose(PR.disagreement(preds).numpy(), g["disc"], rtol=1e-4)


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_fp64_restatement_matches_the_reference_train_step(golden, golden_path, optim):
    """One DynamicsModel.train_step (grad_clip 1.0, a fresh optimizer) of the reference in fp64
    against plain_ref.train_step: the loss and every updated parameter to fp64 rounding."""
    g = golden("g24_plain.npz")
    sd = _ckpt(golden_path)[0]["model"]
    tr, norms = _norms(g)
    idx = torch.as_tensor(g["step_idx"], dtype=torch.long)
    lr, p1 = ((float(g["adam_lr0"]), float(g["adam_eps0"])) if optim == "adam" else
              (float(g["f64_sgd_lr"]), float(g["f64_sgd_momentum"])))
    loss, new = PR.train_step(sd, norms, tuple(x[idx] for x in tr), optim, lr, p1, 1.0)
    assert abs(loss - float(g[f"f64_{optim}_loss"])) <= 1e-13 * abs(loss)
    moved = 0.0
    for j, (k, v) in enumerate(new.items()):
        ref = g[f"f64_{optim}_p{j}"]
        assert v.dtype == torch.float64 and ref.dtype == np.float64
        # Adam's first step is lr * g / (|g| + eps): relative rounding of g reaches the update
        assert np.abs(v.numpy() - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), k
        moved = max(moved, float(np.abs(ref - sd[k].double().numpy()).max()))
    assert moved > 1e-4  # the step moved the parameters
