"""The data-parallel pieces of the NPG update in one process: the pass with a divisor other than
its own row count (amx_npg_pass_dp / amx_npg_pass_cg_dp), the message path of the CG
(amx_npg_reduce_gated -> all-reduce -> amx_npg_cg_reduce on one block) with an identity all-reduce
against the plain update, bit for bit, and the whitening in two halves (amx_adv_whiten_parts /
amx_adv_whiten_apply).  Two ranks over gloo: tests/test_gpu_npg_dp_ranks.py.

Shapes: the flagship S = 197, A = 36 (npg_pass_ref.S1 / A1) on npg_pass_ref.inputs; the divisor
cases run (rows_per_block, N) = (32, 1), (32, 17), (32, 549) (18 blocks: the two-stage reduce) and
(96, 200) (three chunks per block, a ragged last block).

The message-path cases run DeviceNPG's own rows_per_block, which is 32 below 8193 rows: N = 544 is
17 blocks (a second run of 16 in the reduce), N = 4128 is 129 blocks (9 runs), every block one
chunk.  A block of more than one chunk is reached by the case that forces rows_per_block = 96 at
N = 544 (6 blocks of three chunks, the last ragged).
"""
import numpy as np
import pytest
import torch

import npg_pass_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
VPG, FVP, EVAL = P.VPG, P.FVP, P.EVAL
S, A = P.S1, P.A1
SENTINEL = 7.0
DIV_CASES = [(32, 1), (32, 17), (32, 549), (96, 200)]

_CTX, _PART = {}, {}


def ctx():
    import amp_extensions_amd as amx
    if "c" not in _CTX:
        _CTX["c"] = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV)
    return _CTX["c"]


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(x):
    """The bit pattern of a float / array / tensor (NaN compares by payload)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(np.asarray(x))
    return x.view({8: np.uint64, 4: np.uint32}[x.dtype.itemsize])


def launch(mode, rpb, N, n_total=None, hcache=None, expect_error=False):
    """One pass on npg_pass_ref.inputs into a NaN-filled [blocks][W] buffer followed by a sentinel
    row: amx_npg_pass_ex (n_total None) or amx_npg_pass_dp.  Returns the partials as numpy."""
    from amp_extensions_amd import _native as Nn
    c, d = ctx(), P.inputs(S, A, N)
    Pn = P.param_count(S, A)
    W = 2 if mode == EVAL else Pn
    nb = (N + rpb - 1) // rpb
    buf = torch.full((nb * W + Pn,), SENTINEL, dtype=torch.float64, device=DEV)
    buf[:nb * W] = float("nan")
    obs, act, adv = to_dev(d["obs"]), to_dev(d["act"]), to_dev(d["adv"])
    theta, vec = to_dev(d["theta"]), to_dev(P.mode_vec(d, mode))
    args = (c.h, mode, N, obs.data_ptr(), Nn.AMX_IN_F32, obs.stride(0), act.data_ptr(), Nn.AMX_IN_F32,
            act.stride(0), adv.data_ptr(), theta.data_ptr(), ptr(vec), rpb, buf.data_ptr(), None, ptr(hcache))
    if n_total is None:
        rc = c.lib.amx_npg_pass_ex(*args, c.stream)
    else:
        rc = c.lib.amx_npg_pass_dp(*args, n_total, c.stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    if expect_error:
        return rc, out
    assert rc == 0, c.lib.amx_last_error().decode()
    assert not np.isnan(out[:nb * W]).any(), "an element of the partials was not written"
    assert (out[nb * W:] == SENTINEL).all(), "the pass wrote past [blocks][W]"
    return out[:nb * W].reshape(nb, W)


def plain(mode, rpb, N):
    """amx_npg_pass_ex's partials: once per case, shared, read-only."""
    key = (mode, rpb, N)
    if key not in _PART:
        _PART[key] = launch(mode, rpb, N)
        _PART[key].setflags(write=False)
    return _PART[key]


def written_hcache(rpb, N):
    hc = torch.full((N, 64), float("nan"), dtype=torch.float32, device=DEV)
    launch(VPG, rpb, N, hcache=hc)
    assert not torch.isnan(hc).any()
    return hc


# ---- 1. the divisor ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,hc", [(VPG, False), (VPG, True), (FVP, False), (FVP, True), (EVAL, False)],
                         ids=["VPG", "VPG-hcache", "FVP", "FVP-hcache", "EVAL"])
@pytest.mark.parametrize("rpb,N", DIV_CASES)
def test_divisor_equal_to_rows_is_pass_ex(mode, hc, rpb, N):
    """n_total == N: amx_npg_pass_ex bit for bit (EVAL takes no hcache: the pass refuses one)."""
    hcache = None
    if hc:  # VPG writes it (and must write the same rows); FVP reads the rows a VPG pass wrote
        hcache = torch.full((N, 64), float("nan"), dtype=torch.float32, device=DEV) if mode == VPG \
            else written_hcache(rpb, N)
    got = launch(mode, rpb, N, n_total=N, hcache=hcache)
    assert np.array_equal(bits(got), bits(plain(mode, rpb, N)))
    if hc and mode == VPG:
        assert torch.equal(hcache, written_hcache(rpb, N))


@pytest.mark.parametrize("mode,hc", [(VPG, False), (FVP, False), (FVP, True)], ids=["VPG", "FVP", "FVP-hcache"])
@pytest.mark.parametrize("rpb,N", DIV_CASES)
def test_divisor_twice_the_rows_halves_every_partial(mode, hc, rpb, N):
    """1 / (2 N) is half of 1 / N exactly and a power of two commutes with every rounding of the
    pass (the inputs' magnitudes are far from underflow): every partial is exactly half."""
    got = launch(mode, rpb, N, n_total=2 * N, hcache=written_hcache(rpb, N) if hc else None)
    want = 0.5 * plain(mode, rpb, N)
    assert np.abs(want).max() > 0
    assert np.array_equal(bits(got), bits(want)), float(np.abs(got - want).max())


@pytest.mark.parametrize("rpb,N", DIV_CASES)
def test_eval_sums_do_not_depend_on_the_divisor(rpb, N):
    assert np.array_equal(bits(launch(EVAL, rpb, N, n_total=3 * N + 5)), bits(plain(EVAL, rpb, N)))


@pytest.mark.parametrize("mode", [VPG, FVP], ids=["VPG", "FVP"])
@pytest.mark.parametrize("rpb,N", DIV_CASES)
def test_divisor_not_a_power_of_two_vs_reference(mode, rpb, N):
    """n_total = 3 N + 5 against npg_pass_ref.pass_ref(N = n_total) per block, for the column sum
    and for a short last block with the one before it: tests/test_gpu_npg_pass.py's measure
    (|x - ref| / (2^-24 mag) per parameter block) and allowance (K15 from 15 rows on, K below)."""
    n_total = 3 * N + 5
    d = P.inputs(S, A, N)
    part = launch(mode, rpb, N, n_total=n_total)
    blocks = P.block_ranges(rpb, N)
    ranges = [(("block", b), r0, r1, part[b]) for b, (r0, r1) in enumerate(blocks)] + [("sum", 0, N, part.sum(0))]
    if len(blocks) > 1 and blocks[-1][1] - blocks[-1][0] < P.MANY_ROWS:
        ranges.append(("last two blocks", blocks[-2][0], N, part[-2] + part[-1]))
    fails, worst = [], 0.0
    for name, r0, r1, x in ranges:
        ref, mag = P.pass_ref(mode, S, A, d["theta"], d["obs"], d["act"], d["adv"], P.mode_vec(d, mode), n_total,
                              r0, r1)
        k = P.allowance(mode, r1 - r0)
        for seg, v in P.segment_max(P.ratio(x, ref, mag), S, A).items():
            worst = max(worst, v / k)
            if not v <= k:
                fails.append((name, (r0, r1), seg, round(v, 1), k))
    print(f"DIVISOR {P.MODE_NAMES[mode]} rpb={rpb} N={N} n_total={n_total}: worst ratio / allowance {worst:.3f}")
    assert not fails, fails


def test_invalid_divisor_is_an_error_and_launches_nothing():
    c = ctx()
    for n_total in (548, 0, -3):
        rc, out = launch(VPG, 32, 549, n_total=n_total, expect_error=True)
        assert rc != 0 and b"n_total" in c.lib.amx_last_error()
        assert np.isnan(out[:18 * P.param_count(S, A)]).all(), "the refused pass wrote partials"
    # the folded pass: the same refusal (the fold's operands are valid: only n_total is wrong)
    Pn = P.param_count(S, A)
    d = P.inputs(S, A, 549)
    obs, theta = to_dev(d["obs"]), to_dev(d["theta"])
    f64 = [torch.zeros(Pn, dtype=torch.float64, device=DEV) for _ in range(5)]
    p32 = torch.zeros(Pn, dtype=torch.float32, device=DEV)
    st = [torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2)]
    work = torch.zeros(int(c.lib.amx_npg_cg_tail_work(Pn)), dtype=torch.float64, device=DEV)
    part = torch.full((18, Pn), float("nan"), dtype=torch.float64, device=DEV)
    from amp_extensions_amd import _native as Nn
    rc = c.lib.amx_npg_pass_cg_dp(c.h, 549, obs.data_ptr(), Nn.AMX_IN_F32, obs.stride(0), theta.data_ptr(), 32,
                                  part.data_ptr(), None, 0.0, f64[0].data_ptr(), f64[1].data_ptr(),
                                  f64[2].data_ptr(), f64[3].data_ptr(), f64[4].data_ptr(), p32.data_ptr(),
                                  st[0].data_ptr(), st[1].data_ptr(), work.data_ptr(), 548, c.stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"n_total" in c.lib.amx_last_error()
    assert torch.isnan(part).all()


# ---- 2. the message path with an identity all-reduce ------------------------------------------
GLOBAL_KEYS = ("vpg_grad", "npg_grad", "alpha", "delta", "surr_after", "kl_dist")


def make_npg(N, rpb=None, **kw):
    import amp_extensions_amd as amx
    from amp_extensions_amd.npg import unpack_policy
    d = P.inputs(S, A, N)
    layers, ls = unpack_policy(d["theta"], S, A)
    kw.setdefault("FIM_invert_args", {"iters": 10, "damping": 1e-4})
    npg = amx.DeviceNPG(ctx(), layers, ls, normalized_step_size=0.05, min_log_std=-2.0, **kw)
    if rpb is not None:
        npg._rows_per_block = lambda n: rpb
    return npg, d


def update(N, whiten, dp, rpb=None, **kw):
    npg, d = make_npg(N, rpb, **kw)
    calls = []

    def identity(t):
        calls.append(tuple(t.shape))
        return t
    extra = dict(allreduce=identity, rank=0, world=1) if dp else {}
    out = npg.train_from_arrays(d["obs"], d["act"], d["adv"], whiten=whiten, **extra)
    torch.cuda.synchronize()
    out["theta"] = npg.theta
    return out, calls


def assert_same_update(a, b):
    for k in GLOBAL_KEYS + ("advantages", "theta"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("whiten", [True, False], ids=["whiten", "raw"])
@pytest.mark.parametrize("N", [1, 33, 512, 544, 4128])
def test_message_path_identity_allreduce_bit_identical(N, whiten):
    """train_from_arrays through the message path (one rank, an all-reduce that changes nothing)
    against the plain update: theta and every entry of the result, bit for bit."""
    want, _ = update(N, whiten, dp=False)
    got, calls = update(N, whiten, dp=True)
    Pn = P.param_count(S, A)
    assert calls == [(1,)] + ([(1, 4)] if whiten else []) + [(Pn,)] * 11 + [(2,)]
    assert_same_update(got, want)
    assert got["n_total"] == N
    if N > 1:  # (one whitened row is 0 / 1e-6: the update is NaN on both paths, the same NaN)
        assert np.isfinite(got["theta"].cpu().numpy()).all() and not torch.equal(got["theta"], to_dev(
            P.inputs(S, A, N)["theta"]))


def test_message_path_multi_chunk_blocks_bit_identical():
    """rows_per_block = 96 at N = 544: six blocks of three chunks (the last ragged)."""
    want, _ = update(544, True, dp=False, rpb=96)
    got, _ = update(544, True, dp=True, rpb=96)
    assert_same_update(got, want)


def test_message_path_early_stop_bit_identical():
    """A solve that stops before its last iteration: the later passes, messages and column sums
    sit behind the gate, and the message buffer keeps being all-reduced.  residual_tol is twice the
    true residual |b - (F + damping) x_4|^2 of the 4-iteration solve, so the recursion's r.r falls
    below it at iteration 4 at the latest; that it stopped is checked against the full solve."""
    N = 544
    npg, d = make_npg(N, FIM_invert_args={"iters": 4, "damping": 1e-4}, residual_tol=0.0)
    o, a, adv = npg._inputs(d["obs"], d["act"], d["adv"])
    b = npg.flat_vpg(o, a, adv)
    x4 = npg.cg_solve(o, a, b)
    tol = 2.0 * float(((b - npg.HVP(o, a, x4)) ** 2).sum())
    assert tol > 0
    full, _ = update(N, False, dp=False, residual_tol=0.0)
    want, _ = update(N, False, dp=False, residual_tol=tol)
    got, calls = update(N, False, dp=True, residual_tol=tol)
    assert not torch.equal(want["npg_grad"], full["npg_grad"]), "the solve did not stop early"
    assert len(calls) == 1 + 1 + 10 + 1  # the host still runs every collective
    assert_same_update(got, want)
    # a solve stopped by its first step (everything after iteration 1 is gated)
    want, _ = update(N, True, dp=False, residual_tol=1e30)
    got, _ = update(N, True, dp=True, residual_tol=1e30)
    assert_same_update(got, want)


_PLAIN = {}


@pytest.mark.parametrize("option", ["eval_before", "dist_info"])
@pytest.mark.parametrize("N,rpb", [(33, None), (544, 96)], ids=["33", "544-rpb96"])
def test_eval_before_or_dist_info_alone_changes_no_bit_of_the_update(N, rpb, option):
    """eval_before alone, or dist_info alone, adds launches (surr_before's EVAL pass, the per-row
    log-likelihoods) but no arithmetic to the update: the gradients, the step, surr_after, kl_dist
    and the new theta are the plain update's from the same start, bit for bit."""
    if (N, rpb) not in _PLAIN:
        _PLAIN[N, rpb] = update(N, True, dp=False, rpb=rpb)[0]
    want = _PLAIN[N, rpb]
    assert want["surr_before"] == 0.0 and "hvp_products" not in want and "lr" not in want
    npg, d = make_npg(N, rpb)
    npg.eval_before = option == "eval_before"
    got = npg.train_from_arrays(d["obs"], d["act"], d["adv"], dist_info=option == "dist_info")
    torch.cuda.synchronize()
    got["theta"] = npg.theta
    assert got["hvp_products"] == 0 and ("lr" in got) == (option == "dist_info")
    assert_same_update(got, want)
    assert np.isfinite(got["theta"].cpu().numpy()).all() and not torch.equal(got["theta"], to_dev(d["theta"]))


# ---- 3. the whitening in two halves -----------------------------------------------------------
def whiten_parts(adv, lo, hi, rank, world, msg):
    c = ctx()
    n = hi - lo
    rc = c.lib.amx_adv_whiten_parts(c.h, 1, n, None, None, n, adv.data_ptr() + 8 * lo, rank, world, msg.data_ptr(),
                                    c.stream)
    assert rc == 0, c.lib.amx_last_error().decode()


def whiten_apply(adv, lo, hi, msg, world):
    c = ctx()
    n = hi - lo
    out = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    stats = torch.empty(2, dtype=torch.float64, device=DEV)
    rc = c.lib.amx_adv_whiten_apply(c.h, 1, n, None, None, n, adv.data_ptr() + 8 * lo, msg.data_ptr(), world, 1e-6,
                                    out.data_ptr(), stats.data_ptr(), c.stream)
    assert rc == 0, c.lib.amx_last_error().decode()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[n] == SENTINEL
    return o[:n], stats.cpu().numpy()


@pytest.mark.parametrize("order", [(1, 31, 500), (500, 1, 31)], ids=["1-31-500", "500-1-31"])
def test_whiten_halves_three_slots(order):
    """Three slots filled in one process (the zeroed [3][4] message after the SUM all-reduce is the
    three records side by side): stats against numpy's two-pass fp64 over the union within 1e-12
    relative; every applied row within 1 fp64 ulp of (adv - mean) / (std + 1e-6) formed from the
    device's own stats."""
    x = np.random.RandomState(3).randn(sum(order)) * 1.5 + 0.2
    adv = to_dev(x)
    msg = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    edges = np.concatenate([[0], np.cumsum(order)])
    for r in range(3):
        whiten_parts(adv, int(edges[r]), int(edges[r + 1]), r, 3, msg)
    rec = msg.cpu().numpy()
    assert rec[:, 0].tolist() == [float(n) for n in order]
    all_stats = []
    for r in range(3):
        lo, hi = int(edges[r]), int(edges[r + 1])
        rows, stats = whiten_apply(adv, lo, hi, msg, 3)
        all_stats.append(stats)
        want = (x[lo:hi] - stats[0]) / (stats[1] + 1e-6)
        assert (np.abs(rows - want) <= np.spacing(np.abs(want))).all()
    assert all(np.array_equal(bits(s), bits(all_stats[0])) for s in all_stats)
    mean, std = x.mean(), x.std()
    print(f"WHITEN3 mean rel {abs(all_stats[0][0] - mean) / abs(mean):.2e} std rel {abs(all_stats[0][1] - std) / std:.2e}")
    assert abs(all_stats[0][0] - mean) <= 1e-12 * abs(mean)
    assert abs(all_stats[0][1] - std) <= 1e-12 * std


@pytest.mark.parametrize("shift", [0.2, 1e6], ids=["mean0.2", "mean1e6"])
@pytest.mark.parametrize("n", [1, 17, 4097, 40960])
def test_whiten_halves_one_slot_is_adv_whiten(n, shift):
    """world = 1: the halves give amx_adv_whiten's stats and rows bit for bit (one block, two
    blocks with a one-element second, ten blocks; a mean far from the spread, where the record's
    residual is not zero)."""
    c = ctx()
    x = np.random.RandomState(n).randn(n) * 1.5 + shift
    adv = to_dev(x)
    want = torch.empty(n, dtype=torch.float64, device=DEV)
    wstats = torch.empty(2, dtype=torch.float64, device=DEV)
    assert c.lib.amx_adv_whiten(c.h, 1, n, None, None, n, adv.data_ptr(), 1e-6, want.data_ptr(), wstats.data_ptr(),
                                c.stream) == 0
    msg = torch.zeros(1, 4, dtype=torch.float64, device=DEV)
    whiten_parts(adv, 0, n, 0, 1, msg)
    rows, stats = whiten_apply(adv, 0, n, msg, 1)
    assert np.array_equal(bits(stats), bits(wstats))
    assert np.array_equal(bits(rows), bits(want))
