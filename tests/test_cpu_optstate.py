"""CPU-only checks of amp_extensions_amd/optstate.py: the one description of where the device
fits keep each nn.Linear tensor in their padded flat vectors (ParamLayout), and the one path
between torch.optim state and those vectors.  Every shape here has live sizes strictly smaller
than the padded ones, so every slice is exercised."""

import pytest
import torch
import torch.nn as nn

from amp_extensions_amd import _build, _native
from amp_extensions_amd import optstate as O

# the ensemble case: S, A, hidden, L (two members: the stacked vectors of test_padding_and_views)
# and what AmxContext derives from them
# (k0_pad = round_up(S + A, 32), Hp = round_up(hidden, 128), ldk = k0_pad + L Hp, n_out_pad = round_up(S, 128))
ES, EA, EH, EL = 3, 2, 4, 2
K0, HP, LDK, NOUT = 32, 128, 288, 128

LAYOUTS = {
    "baseline": lambda: O.baseline_layout(21, 32, (5, 7), (128, 128)),     # S + 4 = 21
    "disc": lambda: O.disc_layout(10, 32, (6, 9), (128, 128)),
    "policy": lambda: O.policy_layout(5, 3),
    "ensemble": lambda: O.ensemble_layout(ES, EA, EH, EL, K0, HP, LDK, NOUT),
}
OPTIMIZERS = {
    "adam": lambda p: torch.optim.Adam(p, lr=1e-2),
    "sgd": lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9),
    "nesterov": lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9, nesterov=True),
}


@pytest.fixture(scope="module")
def lib():
    return _native.load(_build.build(verbose=False))


def make_model(layout, seed=0):
    """An nn.Sequential of Linear layers with the layout's live shapes (a parameter container: the
    ensemble's dense-connect layers do not chain) and, for the policy, log_std behind it."""
    torch.manual_seed(seed)
    live = layout.live
    model = nn.Sequential(*[nn.Linear(w[1], w[0]) for w in live[0:len(live) // 2 * 2:2]])
    extra = [nn.Parameter(torch.randn(s)) for s in live[len(live) // 2 * 2:]]
    params = list(model.parameters()) + extra
    assert [tuple(p.shape) for p in params] == live
    return model, params


def take_steps(params, opt, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    targets = [torch.randn(p.shape, generator=g) for p in params]
    for _ in range(n):
        opt.zero_grad()
        sum(((p - t) ** 2).sum() for p, t in zip(params, targets)).backward()
        opt.step()


def test_sizes_match_the_library(lib):
    assert LAYOUTS["baseline"]().size == lib.amx_vfit_param_count(32, 128, 128)
    assert LAYOUTS["disc"]().size == lib.amx_dfit_param_count(32, 128, 128)
    assert LAYOUTS["policy"]().size == lib.amx_npg_param_count(5, 3)
    # amx_efit.hip's make_plan: per layer N K weights then N biases, N x K = Hp x (k0_pad + i Hp), last n_out_pad x ldk
    want, offs = 0, []
    for i in range(EL + 1):
        n, k = (NOUT, LDK) if i == EL else (HP, K0 + i * HP)
        offs += [want, want + n * k]
        want += n * k + n
    lay = LAYOUTS["ensemble"]()
    assert lay.size == want and lay.offsets == offs


@pytest.mark.parametrize("source", ["object", "state_dict"])
@pytest.mark.parametrize("name,optim", [("baseline", "adam"), ("disc", "adam"), ("disc", "sgd"), ("policy", "adam"),
                                        ("ensemble", "adam"), ("ensemble", "nesterov")])
def test_round_trip_through_torch_state(name, optim, source):
    layout = LAYOUTS[name]()
    _, params = make_model(layout)
    opt = OPTIMIZERS[optim](params)
    take_steps(params, opt, 3)
    kind, hyper, states = O.read_state(opt if source == "object" else opt.state_dict())
    assert kind == ("adam" if optim == "adam" else "sgd") and hyper["lr"] == 1e-2 and "params" not in hyper
    step = O.common_step(states)
    assert step == (3 if kind == "adam" else 0)
    s1, s2 = O.pack_state(layout, kind, states)
    mask = layout.live_mask()
    assert (s2 is None) == (kind == "sgd")
    for s in (s1,) if s2 is None else (s1, s2):
        assert s.dtype == torch.float32 and tuple(s.shape) == (layout.size,)
        assert not s[~mask].any() and s[mask].all()
    params2 = [nn.Parameter(p.detach().clone()) for p in params]
    opt2 = OPTIMIZERS[optim](params2)
    O.write_state(opt2, kind, step, layout.unpack(s1), None if s2 is None else layout.unpack(s2))
    take_steps(params, opt, 1)
    take_steps(params2, opt2, 1)
    assert all(torch.equal(a, b) for a, b in zip(params, params2))
    assert all(set(opt.state[a]) == set(opt2.state[b]) for a, b in zip(params, params2))


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_padding_and_views(name):
    layout = LAYOUTS[name]()
    live = sum(torch.Size(s).numel() for s in layout.live)
    assert live < layout.size or name == "policy"
    packed = layout.pack([torch.ones(s) for s in layout.live])
    assert packed.sum() == live and set(packed.tolist()) <= {0.0, 1.0}
    mask = layout.live_mask()
    assert mask.dtype == torch.bool and torch.equal(mask, packed.bool())
    # views alias the flat vector, with or without a leading member dimension
    stacked = torch.stack([packed, 2 * packed])
    for flat in (packed, stacked):
        views = layout.views(flat)
        assert [tuple(v.shape[flat.dim() - 1:]) for v in views] == layout.padded
        assert all(v.data_ptr() == flat.data_ptr() + 4 * o for v, o in zip(views, layout.offsets))
    assert all(torch.equal(2 * a, b[1]) for a, b in zip(layout.views(packed), layout.views(stacked)))
    # unpack inverts pack and returns clones
    g = torch.Generator().manual_seed(3)
    tensors = [torch.randn(s, generator=g) for s in layout.live]
    flat = layout.pack(tensors)
    back = layout.unpack(flat)
    assert all(torch.equal(a, b) for a, b in zip(tensors, back))
    back[0].zero_()
    assert torch.equal(layout.unpack(flat)[0], tensors[0])


def test_ensemble_columns_follow_the_dense_concat_row():
    layout = LAYOUTS["ensemble"]()
    tensors = [torch.arange(1, torch.Size(s).numel() + 1, dtype=torch.float32).reshape(s) for s in layout.live]
    views = layout.views(layout.pack(tensors))
    for i in range(EL + 1):
        W, Wp = tensors[2 * i], views[2 * i]
        assert tuple(W.shape) == (ES if i == EL else EH, ES + EA + i * EH)
        for j in range(W.shape[1]):  # input j: the (s, a) block, then hidden layer (j - S - A) // hidden's block
            col = j if j < ES + EA else K0 + (j - ES - EA) // EH * HP + (j - ES - EA) % EH
            assert torch.equal(Wp[:W.shape[0], col], W[:, j])
        assert Wp.count_nonzero() == W.numel()
        assert torch.equal(views[2 * i + 1][:W.shape[0]], tensors[2 * i + 1])


def test_shape_errors_name_both_shapes():
    layout = LAYOUTS["baseline"]()
    tensors = [torch.ones(s) for s in layout.live]
    tensors[2] = torch.ones(7, 6)
    with pytest.raises(ValueError, match=r"expected .*\(7, 5\).* found .*\(7, 6\)"):
        layout.pack(tensors)
    with pytest.raises(ValueError):
        layout.pack(tensors[:-1])
    with pytest.raises(ValueError):
        layout.views(torch.zeros(layout.size + 1))


REFUSED = {
    "amsgrad": lambda p: torch.optim.Adam(p, amsgrad=True),
    "maximize": lambda p: torch.optim.Adam(p, maximize=True),
    "sgd_maximize": lambda p: torch.optim.SGD(p, lr=0.1, momentum=0.9, maximize=True),
    "two_groups": lambda p: torch.optim.Adam([{"params": p[:2]}, {"params": p[2:]}]),
    "dampening": lambda p: torch.optim.SGD(p, lr=0.1, momentum=0.9, dampening=0.1),
    "rmsprop": lambda p: torch.optim.RMSprop(p, momentum=0.9),
    "adamw": lambda p: torch.optim.AdamW(p),   # its state_dict has Adam's keys
}


@pytest.mark.parametrize("source", ["object", "state_dict"])
@pytest.mark.parametrize("what", list(REFUSED))
def test_unsupported_optimizers_are_refused(what, source):
    _, params = make_model(LAYOUTS["baseline"]())
    opt = REFUSED[what](params)
    with pytest.raises(NotImplementedError):
        O.read_state(opt if source == "object" else opt.state_dict())


def test_only_the_asked_kinds_pass():
    _, params = make_model(LAYOUTS["baseline"]())
    with pytest.raises(NotImplementedError, match="SGD"):
        O.read_state(torch.optim.SGD(params, lr=0.1), kinds=("adam",))
    assert O.read_state(torch.optim.Adam(params), kinds=("adam",))[0] == "adam"


def two_speed_optimizer(params):
    """Adam whose first parameter has taken one step more than the others."""
    opt = torch.optim.Adam(params, lr=1e-2)
    opt.zero_grad()
    (params[0] ** 2).sum().backward()
    opt.step()
    take_steps(params, opt, 1)
    return opt


def test_different_steps_and_wrong_shapes_write_nothing():
    layout = LAYOUTS["baseline"]()
    _, params = make_model(layout)
    kind, _, states = O.read_state(two_speed_optimizer(params))
    assert [s[0] for s in states] == [2, 1, 1, 1, 1, 1]
    with pytest.raises(NotImplementedError, match="different"):
        O.common_step(states)
    # parameters without state do not vote, and load as zeros
    fresh = [states[0]] + [(0, None, None)] * 5
    assert O.common_step(fresh) == 2 and O.common_step([(0, None, None)] * 6) == 0
    s1, s2 = O.pack_state(layout, kind, fresh)
    assert torch.equal(layout.unpack(s1)[0], states[0][1]) and not any(t.any() for t in layout.unpack(s1)[1:])
    # a state tensor of the wrong shape
    bad = list(states)
    bad[3] = (1, torch.ones(8), torch.ones(8))
    with pytest.raises(ValueError, match=r"expected .*\(7,\).* found .*\(8,\)"):
        O.pack_state(layout, kind, bad)
    with pytest.raises(ValueError):
        O.pack_state(layout, kind, states[:-1])
    opt = torch.optim.Adam(params)
    m = [s[1] for s in states]
    with pytest.raises(ValueError):
        O.write_state(opt, "adam", 1, m[:3] + [torch.ones(8)] + m[4:], m)
    assert not opt.state


def test_baseline_refusals_need_no_gpu():
    """DeviceMLPBaseline.from_mjrl / load_optimizer refuse what the device Adam does not implement
    (it used to train these as plain Adam on group 0) from the optimizer alone."""
    from amp_extensions_amd.gae import DeviceMLPBaseline
    layout = O.baseline_layout(21, 32, (5, 7), (128, 128))
    model, params = make_model(layout)

    class Baseline:
        batch_size, epochs = 64, 1

    bl = DeviceMLPBaseline.__new__(DeviceMLPBaseline)
    bl.widths, bl.batch_size, bl.layout = [5, 7], 64, layout
    for make in (REFUSED["maximize"], REFUSED["amsgrad"], REFUSED["two_groups"], REFUSED["rmsprop"],
                 OPTIMIZERS["sgd"], two_speed_optimizer):
        mj = Baseline()
        mj.model, mj.optimizer = model, make(params)
        with pytest.raises(NotImplementedError):
            bl.load_optimizer(mj.optimizer)
        if make is not two_speed_optimizer:
            with pytest.raises(NotImplementedError):
                DeviceMLPBaseline.from_mjrl(None, mj)
