"""The data-parallel NPG update without a GPU: the rank-order combine of the whitening records
restated in numpy, the collective schedule of one update (a recording all-reduce over a stubbed
native layer: every native call returns success and leaves its buffers alone, so only the order,
count and shapes of the messages and launches are pinned here; the numbers are the GPU tests'),
the native calls of every variant of the one update body in order, and dist.rank_world."""
import numpy as np
import pytest
import torch

import npg_pass_ref as P


# ---- 1. the combine of {count, mean, M2, residual} records -------------------------------------
def combine(parts):
    """k_whiten_apply's combine of (n, m, M2, R) parts in order, as the kernel writes it."""
    n = dev = a = 0.0
    have = False
    for nb, m, _, r in parts:
        if nb > 0.0:
            if not have:
                a = m
            have = True
            n += nb
            dev += r + nb * (m - a)
    mean = a + dev / n if n > 0.0 else 0.0
    m2 = 0.0
    for nb, m, q, r in parts:
        d = m - mean
        m2 += q + (2.0 * d * r + nb * d * d)
    return n, mean, m2


def block_part(x):
    """k_whiten_part on one chunk (the sums in numpy's order: the order is not what is pinned)."""
    n = float(x.size)
    m = x.sum() / n if n else 0.0
    d = x - m
    return n, m, float((d * d).sum()), float(d.sum())


def rank_record(x, ch=4096):
    """amx_adv_whiten_parts: the chunks' parts combined, the residual about the combined mean."""
    parts = [block_part(x[i:i + ch]) for i in range(0, max(x.size, 1), ch)]
    n, mean, m2 = combine(parts)
    res = 0.0
    for nb, m, _, r in parts:
        if nb > 0.0:
            res += r + nb * (m - mean)
    for _ in range(64):
        if not (n > 0.0 and mean + res / n != mean):
            break
        res *= 0.5
    return n, mean, m2, res


@pytest.mark.parametrize("shift", [0.2, 1e6])
@pytest.mark.parametrize("split", [(1, 31, 500), (500, 1, 31), (5000, 1), (1, 1, 1), (4097, 3, 9000), (64,)])
def test_rank_order_combine_matches_two_pass(split, shift):
    x = np.random.RandomState(sum(split)).randn(sum(split)) * 1.5 + shift
    edges = np.concatenate([[0], np.cumsum(split)])
    recs = [rank_record(x[edges[r]:edges[r + 1]]) for r in range(len(split))]
    n, mean, m2 = combine(recs)
    std = np.sqrt(m2 / n)
    assert n == x.size
    assert abs(mean - x.mean()) <= 1e-12 * abs(x.mean())
    assert abs(std - x.std()) <= 1e-12 * x.std()
    # a single record is a fixed point of the combine: amx_adv_whiten's stats bit for bit
    one = rank_record(x)
    n1, mean1, m21 = combine([one])
    assert (n1, mean1, m21) == one[:3]


# ---- 2. the collective schedule ------------------------------------------------------------------
S, A = 5, 3


class _Lib:
    def __init__(self, log, trace=None):
        self.log, self.trace = log, trace

    def __getattr__(self, name):
        def call(*args):
            self.log.append(name)
            if self.trace is not None:  # the pass entry points with their mode argument
                self.trace.append(f"{name}:{args[1]}" if name in ("amx_npg_pass_ex", "amx_npg_pass_dp") else name)
            if name == "amx_npg_param_count":
                return P.param_count(args[0], args[1])
            if name == "amx_npg_cg_tail_work":
                return args[0] + (args[0] + 63) // 64
            return 0
        return call


class _Ctx:
    device = torch.device("cpu")
    stream, h = 0, None

    def __init__(self, log, trace=None):
        self.S, self.A, self.lib = S, A, _Lib(log, trace)


def stub_npg(log, iters, trace=None):
    from amp_extensions_amd.npg import DeviceNPG
    layers = [(torch.zeros(32, S), torch.zeros(32)), (torch.zeros(32, 32), torch.zeros(32)),
              (torch.zeros(A, 32), torch.zeros(A))]
    return DeviceNPG(_Ctx(log, trace), layers, torch.zeros(A), FIM_invert_args={"iters": iters, "damping": 1e-4})


@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_collective_schedule(whiten, world, rank):
    iters, n, Pn = 4, 7, P.param_count(S, A)
    log = []
    npg = stub_npg(log, iters)

    def allreduce(t):
        log.append(("allreduce", tuple(t.shape), t.dtype))
        if t.dtype == torch.int64:  # the other ranks' row counts
            assert t.tolist() == [n if r == rank else 0 for r in range(world)]
            t[t == 0] = 11
    del log[:]
    out = npg.train_from_arrays(np.zeros((n, S), np.float32), np.zeros((n, A), np.float32), np.zeros(n),
                                whiten=whiten, allreduce=allreduce, rank=rank, world=world)
    assert out["n_total"] == n + 11 * (world - 1)
    msgs = [e[1:] for e in log if isinstance(e, tuple)]
    f64 = torch.float64
    assert msgs == ([((world,), torch.int64)] + ([((world, 4), f64)] if whiten else []) + [((Pn,), f64)] +
                    [((Pn,), f64)] * iters + [((2,), f64)])
    names = [e if isinstance(e, str) else "allreduce" for e in log]
    want = ["allreduce"]
    if whiten:
        want += ["amx_adv_whiten_parts", "allreduce", "amx_adv_whiten_apply"]
    want += ["amx_npg_pass_dp", "amx_npg_reduce_gated", "allreduce", "amx_npg_cg_init_ls", "amx_npg_cg_tail_work"]
    for it in range(iters):  # pass, the message, the collective, the column sums on the message
        want += ["amx_npg_pass_dp" if it == 0 else "amx_npg_pass_cg_dp", "amx_npg_reduce_gated", "allreduce",
                 "amx_npg_cg_reduce"]
    want += ["amx_npg_cg_xrp", "amx_npg_apply_step", "amx_npg_pass_dp", "amx_npg_reduce_gated", "allreduce"]
    assert names == want


def test_no_allreduce_is_the_plain_update():
    """allreduce=None: the launches of the single-process update, none of the new entry points."""
    log = []
    npg = stub_npg(log, 3)
    del log[:]
    npg.train_from_arrays(np.zeros((7, S), np.float32), np.zeros((7, A), np.float32), np.zeros(7))
    assert log == (["amx_adv_whiten", "amx_npg_pass_ex", "amx_npg_reduce_gated", "amx_npg_cg_init_ls",
                    "amx_npg_cg_tail_work", "amx_npg_pass_ex", "amx_npg_cg_reduce"] +
                   ["amx_npg_pass_cg", "amx_npg_cg_reduce"] * 2 +
                   ["amx_npg_cg_xrp", "amx_npg_apply_step", "amx_npg_pass_ex", "amx_npg_reduce_gated"])


def test_errors_decided_before_or_right_after_the_counts():
    log = []
    npg = stub_npg(log, 2)
    z = (np.zeros((7, S), np.float32), np.zeros((7, A), np.float32), np.zeros(7))
    calls = []

    def allreduce(t):
        calls.append(tuple(t.shape))
    for kw in (dict(bc=(z[0], z[1], 0.1)), dict(dist_info=True), dict(idx=np.zeros((2, 3), np.int32))):
        with pytest.raises(NotImplementedError):
            npg.train_from_arrays(*z, allreduce=allreduce, rank=0, world=2, **kw)
    npg.hvp_subsample = 0.5
    with pytest.raises(NotImplementedError):
        npg.train_from_arrays(*z, allreduce=allreduce, rank=0, world=2)
    npg.hvp_subsample = 1.0
    assert calls == []
    # an empty rank (here: the other one, whose count the stub leaves 0): after the counts, nothing else
    del log[:]
    with pytest.raises(ValueError, match="rank 1 of 2 holds no rows"):
        npg.train_from_arrays(*z, allreduce=allreduce, rank=0, world=2)
    assert calls == [(2,)] and log == []
    with pytest.raises(ValueError):
        npg.train_from_arrays(*z, allreduce=allreduce, rank=2, world=2)


# ---- 2b. every variant of the one update body: its native calls, in order ------------------------
# name -> (attributes set on the DeviceNPG, train_from_arrays' keyword arguments)
_Z4 = (np.zeros((4, S), np.float32), np.zeros((4, A), np.float32), 0.1)
VARIANTS = {
    "plain": ({}, {}),
    "raw": ({}, dict(whiten=False)),
    "cg_iters0": (dict(cg_iters=0), {}),
    "nofold": (dict(cg_fold=False), {}),
    "eval_before": (dict(eval_before=True), {}),
    "dist_info": ({}, dict(dist_info=True)),
    "bc": ({}, dict(bc=_Z4)),
    "idx": ({}, dict(idx=np.arange(6, dtype=np.int32).reshape(3, 2))),
    "sub0.5": (dict(hvp_subsample=0.5), {}),
    "dp-1-0": ({}, dict(world=1, rank=0)),
    "dp-3-1": ({}, dict(world=3, rank=1)),
}
DRAW_SEED = 1234


def run_variant(name):
    """One stubbed update at n = 7, iters = 3: (the native calls and collectives in order, the
    result's keys, hvp_products, numpy's generator state before and after the call)."""
    attrs, kw = VARIANTS[name]
    trace = []
    npg = stub_npg([], 3, trace)
    for k, v in attrs.items():
        setattr(npg, k, v)
    kw = dict(kw)
    if "world" in kw:
        def allreduce(t):
            trace.append("allreduce")
            if t.dtype == torch.int64:
                t[t == 0] = 11
        kw["allreduce"] = allreduce
    np.random.seed(DRAW_SEED)
    before = np.random.get_state()
    del trace[:]
    with np.errstate(all="ignore"):  # the stubbed kernels leave the result buffers uninitialised
        out = npg.train_from_arrays(np.zeros((7, S), np.float32), np.zeros((7, A), np.float32), np.zeros(7), **kw)
    return trace, sorted(out), npg.hvp_products, before, np.random.get_state()


# Recorded on the commit before the three update bodies and the two solves were folded into one
# each: these are that commit's sequences, not the folded code's.
_RED, _INIT = "amx_npg_reduce_gated", ["amx_npg_cg_init_ls", "amx_npg_cg_tail_work"]
_VPG, _BEFORE = ["amx_npg_pass_ex:0", _RED], ["amx_npg_pass_ex:2", _RED]
_SOLVE = _INIT + ["amx_npg_pass_ex:1", "amx_npg_cg_reduce"] + ["amx_npg_pass_cg", "amx_npg_cg_reduce"] * 2 + \
    ["amx_npg_cg_xrp"]
_SOLVE_IDX = _INIT + ["amx_npg_pass_idx", "amx_npg_cg_reduce"] + ["amx_npg_pass_cg_idx", "amx_npg_cg_reduce"] * 2 + \
    ["amx_npg_cg_xrp"]
_END = ["amx_npg_apply_step", "amx_npg_pass_ex:2", _RED]
_LL = ["amx_npg_ll_blocks", "amx_npg_ll", _RED]
_DP = (["allreduce", "amx_adv_whiten_parts", "allreduce", "amx_adv_whiten_apply", "amx_npg_pass_dp:0", _RED,
        "allreduce"] + _INIT + ["amx_npg_pass_dp:1", _RED, "allreduce", "amx_npg_cg_reduce"] +
       ["amx_npg_pass_cg_dp", _RED, "allreduce", "amx_npg_cg_reduce"] * 2 +
       ["amx_npg_cg_xrp", "amx_npg_apply_step", "amx_npg_pass_dp:2", _RED, "allreduce"])
_KEYS = ["advantages", "alpha", "delta", "kl_dist", "npg_grad", "surr_after", "surr_before", "vpg_grad"]
_KEYS_EXT = sorted(_KEYS + ["hvp_products"])
WANT = {
    "plain": (["amx_adv_whiten"] + _VPG + _SOLVE + _END, _KEYS),
    "raw": (_VPG + _SOLVE + _END, _KEYS),
    "cg_iters0": (["amx_adv_whiten"] + _VPG + _INIT + _END, _KEYS),
    "nofold": (["amx_adv_whiten"] + _VPG + _INIT + ["amx_npg_pass_ex:1", "amx_npg_cg_tail"] * 3 + _END, _KEYS),
    "eval_before": (["amx_adv_whiten"] + _VPG + _BEFORE + _SOLVE + _END, _KEYS_EXT),
    "dist_info": (["amx_adv_whiten"] + _VPG + _BEFORE + _SOLVE + _END + _LL * 2,
                  sorted(_KEYS_EXT + ["lr", "new_dist_info", "old_dist_info"])),
    "bc": (["amx_adv_whiten", "amx_npg_pass_ex:0", "amx_npg_pass_ex:0", _RED] + _BEFORE + _LL + _SOLVE + _END + _LL,
           _KEYS_EXT),
    "idx": (["amx_adv_whiten"] + _VPG + _BEFORE + _SOLVE_IDX + _END, _KEYS_EXT),
    "sub0.5": (["amx_adv_whiten"] + _VPG + _BEFORE + _SOLVE_IDX + _END, _KEYS_EXT),
    "dp-1-0": (_DP, sorted(_KEYS + ["n_total"])),
    "dp-3-1": (_DP, sorted(_KEYS + ["n_total"])),
}
WANT_STATE = (624, [1234, 3159640283, 4062961311])  # np.random.seed(DRAW_SEED): position, first key words


@pytest.mark.parametrize("name", list(VARIANTS))
def test_native_calls_of_every_variant(name):
    trace, keys, products, before, after = run_variant(name)
    want_trace, want_keys = WANT[name]
    assert trace == want_trace
    assert keys == want_keys
    assert products == 0
    # (the stub's zeroed product counter: the generator is left where it was before any draw)
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and after[2:] == before[2:]
    assert (after[2], after[1][:3].tolist()) == WANT_STATE


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc_layers = torch.nn.ModuleList([torch.nn.Linear(S, 32), torch.nn.Linear(32, 32), torch.nn.Linear(32, A)])
        self.transformations = dict(in_shift=None, in_scale=None, out_shift=None, out_scale=None)


class _Policy:
    """The attributes of mjrl's MLP policy the drop-in reads and writes."""
    min_log_std = -3.0

    def __init__(self):
        self.model, self.log_std = _Model(), torch.zeros(A)
        self.trainable_params = list(self.model.parameters()) + [self.log_std]
        self.old_params = [p.detach().clone() for p in self.trainable_params]
        self.written = None

    def get_param_values(self):
        return np.concatenate([p.detach().numpy().ravel() for p in self.trainable_params])

    def set_param_values(self, new, set_new=True, set_old=True):
        self.written = (np.asarray(new).shape, set_new, set_old)


def test_drop_in_passes_the_allreduce_on():
    """amp_extensions_amd.npg.NPG(..., allreduce=f): raw advantages go to the device (whitened
    there, over the ranks), the schedule is the data-parallel update's, infos carry this rank's
    advantages and no dist-info entries, the parameters are written back."""
    from amp_extensions_amd.npg import NPG
    log, msgs = [], []
    pol = _Policy()
    agent = NPG(None, pol, None, FIM_invert_args={"iters": 2, "damping": 1e-4}, ctx=_Ctx(log),
                allreduce=lambda t: msgs.append(tuple(t.shape)))
    paths = [dict(observations=np.zeros((4, S)), actions=np.zeros((4, A)), advantages=np.arange(4.0),
                  rewards=np.ones(4)) for _ in range(2)]
    infos = {}
    with np.errstate(all="ignore"):  # the stubbed kernels leave the result buffers uninitialised
        stats = agent.train_from_paths(paths, infos)
    Pn = P.param_count(S, A)
    assert msgs == [(1,), (1, 4), (Pn,), (Pn,), (Pn,), (2,)]
    assert "amx_adv_whiten_parts" in log and "amx_adv_whiten" not in log and "amx_npg_ll" not in log
    assert infos["advantages"].shape == (8,) and "old_dist_info" not in infos and infos["surr_before"] == 0.0
    assert pol.written == ((Pn,), True, True) and stats[0] == 4.0 and agent.running_score == 4.0


# ---- 3. dist.rank_world --------------------------------------------------------------------------
def test_rank_world_without_and_with_a_group(tmp_path):
    import torch.distributed as dist

    from amp_extensions_amd import dist as D
    assert not dist.is_initialized() and D.rank_world() == (0, 1)
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        assert D.rank_world() == (0, 1)
        t = torch.ones(3, dtype=torch.float64)
        assert D.allreduce_sum(t) is t and t.tolist() == [1.0, 1.0, 1.0]
    finally:
        dist.destroy_process_group()
    assert D.rank_world() == (0, 1)
