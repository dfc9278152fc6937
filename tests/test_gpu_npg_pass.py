"""The NPG pass kernel (csrc/amx_npg.hip, k_npg) against the plain fp64 reference of one pass
(tests/npg_pass_ref.py), per block and per parameter block, at blocks of one, two, three and five
32-row chunks -- amx_npg_pass_ex / amx_npg_reduce through the C ABI with an explicit
rows_per_block (DeviceNPG's own choice gives one chunk per block below N = 8193).

Every element of every block's partial, and of the reduced vector, must lie within
K * 2^-24 * mag of the reference, mag being the reference's magnitude companion of that element
(so W1 / b1 / W2 / b2 are judged on their own scale, not on b3's) and K the allowance measured on
the CPU from the project's fp32 oracle (npg_pass_ref.K for any range, K15 for ranges of at least
15 rows; tests/test_cpu_npg_pass_ref.py); a last block of fewer rows is also judged at K15 together
with the block before it.  Besides: the shape edges of the tiles and compiled
depths, nothing written outside [blocks][P] and nothing left unwritten, padded and NaN-fenced
inputs, the exact cases (EVAL at new == old on k/64 advantages, FVP's log_std slots, the column
reduction on exactly summable partials), the bit-identity claims of the variants (theta cache,
indexed rows, fp64 and mixed input dtypes, CG fold) re-asserted at three and five chunks per
block, and DeviceNPG.surrogate_kl in the same unit.

Measured on an MI355X (for the record; the bounds are the CPU-measured K15 = 107 / 86 / 3 and
K = 1902 / 10202 / 8 for VPG / FVP / EVAL), the largest ratio |x - ref| / (2^-24 mag) over the
block partials and reduced vectors, ranges of >= 15 rows | fewer:
  BLOCK_CASES, S = 197, A = 36
    VPG   W1 9.9 | 167.0  b1 4.1 | 166.1  W2 7.4 | 668.5  b2 3.0 | 654.2  W3 15.7 | 141.7
          b3 3.8 | 2.4  log_std 1.4 | 1.4
    FVP   W1 14.6 | 230.0  b1 9.7 | 229.1  W2 8.5 | 1376.4  b2 6.8 | 1344.6  W3 10.1 | 387.8
          b3 8.6 | 249.2  log_std 0 | 0
    EVAL  surr 0.2 | 0.4  kl 0.2 | 0.2
  SHAPE_CASES (every range has >= 15 rows)
    VPG   W1 14.7  b1 7.0  W2 8.5  b2 3.8  W3 14.5  b3 3.7  log_std 1.0
    FVP   W1 12.5  b1 18.6  W2 14.0  b2 5.5  W3 8.7  b3 5.8  log_std 0
    EVAL  surr 0.4  kl 0.7
  DeviceNPG.surrogate_kl at N = 200: surr 0.03, kl 0.14.
  The cached activations (VPG's hcache rows), at 3 and at 5 chunks per block: 2.94 (H1) and 2.21
  (H2) fp32 ulps of [0.5, 1) from the fp64 forward; 1.05 and 0.73 ulps of the value from the fp64
  tanh of the kernel's own fp32 sums.  (With layer 1 summed in two fma chains of ~99 terms, as it
  was before these tests, H1 was 4.31 ulps from the fp64 forward: the kernel now sums four.)
The file runs in 3 s (199 tests).
"""
import numpy as np
import pytest
import torch

import npg_pass_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
VPG, FVP, EVAL = P.VPG, P.FVP, P.EVAL
MODES = [VPG, FVP, EVAL]
SENTINEL = 7.0

_CTX, _PART = {}, {}


def ctx_for(S, A):
    import amp_extensions_amd as amx
    if (S, A) not in _CTX:
        _CTX[(S, A)] = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV)
    return _CTX[(S, A)]


def dt(x):
    from amp_extensions_amd import _native as N
    return N.AMX_IN_F64 if x.dtype == torch.float64 else N.AMX_IN_F32


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(c, mode, n, obs, act, adv, theta, vec, rpb, hcache=None, ldo=None, lda=None):
    """One pass into a NaN-filled [blocks][W] buffer followed by a sentinel region one block row of
    P doubles long (W = 2 for EVAL): returns the partials as numpy after checking that every
    element of [blocks][W] was written and nothing after it."""
    Pn = int(c.lib.amx_npg_param_count(c.S, c.A))
    W = 2 if mode == EVAL else Pn
    nb = (n + rpb - 1) // rpb
    buf = torch.full((nb * W + Pn,), SENTINEL, dtype=torch.float64, device=DEV)
    buf[:nb * W] = float("nan")
    rc = c.lib.amx_npg_pass_ex(c.h, mode, n, obs.data_ptr(), dt(obs), obs.stride(0) if ldo is None else ldo,
                               act.data_ptr(), dt(act), act.stride(0) if lda is None else lda, ptr(adv),
                               theta.data_ptr(), ptr(vec), rpb, buf.data_ptr(), None, ptr(hcache), c.stream)
    assert rc == 0, c.lib.amx_last_error().decode()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert not np.isnan(out[:nb * W]).any(), "an element of the partials was not written"
    assert (out[nb * W:] == SENTINEL).all(), "the pass wrote past [blocks][W]"
    return out[:nb * W].reshape(nb, W), buf


def reduce(c, buf, nb, W):
    out = torch.full((W + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    assert c.lib.amx_npg_reduce(c.h, buf.data_ptr(), nb, W, out.data_ptr(), c.stream) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[W] == SENTINEL
    return o[:W]


def device_pass(mode, S, A, rpb, N, exact=False):
    """(partials [blocks][W], reduced [W]) of the plain fp32 pass on npg_pass_ref.inputs: computed
    once per case, shared by the tests.  exact: EVAL with new == old on the k/64 advantages."""
    key = (mode, S, A, rpb, N, exact)
    if key not in _PART:
        d, c = P.inputs(S, A, N), ctx_for(S, A)
        vec = d["theta"] if exact else P.mode_vec(d, mode)
        adv = d["adv_exact"] if exact else d["adv"]
        part, buf = launch(c, mode, N, to_dev(d["obs"]), to_dev(d["act"]), to_dev(adv), to_dev(d["theta"]),
                           to_dev(vec), rpb)
        _PART[key] = (part, reduce(c, buf, part.shape[0], part.shape[1]))
    return _PART[key]


def check_case(mode, S, A, rpb, N):
    """Every block's partial and the reduced vector against the reference; prints the largest ratio
    per segment (>= 15 rows | fewer) and returns the failures."""
    d = P.inputs(S, A, N)
    part, red = device_pass(mode, S, A, rpb, N)
    worst, fails = {}, []
    blocks = P.block_ranges(rpb, N)
    ranges = [(("block", b), r0, r1, part[b]) for b, (r0, r1) in enumerate(blocks)] + [("reduced", 0, N, red)]
    if len(blocks) > 1 and blocks[-1][1] - blocks[-1][0] < P.MANY_ROWS:
        # a last block of a few rows is also judged together with the block before it, at K15
        ranges.append(("last two blocks", blocks[-2][0], N, part[-2] + part[-1]))
    for b, r0, r1, x in ranges:
        ref, mag = P.pass_ref(mode, S, A, d["theta"], d["obs"], d["act"], d["adv"], P.mode_vec(d, mode), N, r0, r1)
        r = P.ratio(x, ref, mag)
        k = P.allowance(mode, r1 - r0)
        tier = int(r1 - r0 < P.MANY_ROWS)
        segs = P.segment_max(r, S, A) if mode != EVAL else {"surr": float(r[0]), "kl": float(r[1])}
        for name, v in segs.items():
            w = worst.setdefault(name, [0.0, 0.0])
            w[tier] = max(w[tier], v)
            if not v <= k:
                fails.append((b, (r0, r1), name, round(v, 1), k))
    print(f"RATIO {P.MODE_NAMES[mode]} S={S} A={A} rpb={rpb} N={N} " +
          " ".join(f"{n}={w[0]:.2f}|{w[1]:.2f}" for n, w in worst.items()))
    return fails


# ---- 1. block partials against the reference ------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=P.MODE_NAMES)
@pytest.mark.parametrize("rpb,N", P.BLOCK_CASES)
def test_block_partials_vs_reference(mode, rpb, N):
    fails = check_case(mode, P.S1, P.A1, rpb, N)
    assert not fails, fails


# ---- 2. shape edges -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=P.MODE_NAMES)
@pytest.mark.parametrize("rpb,N", P.SHAPE_RUNS)
@pytest.mark.parametrize("S,A", P.SHAPE_CASES)
def test_shape_edges_vs_reference(mode, rpb, N, S, A):
    """The ones column that closes a tile or opens a new one (SW = (S + 16) & ~15), every compiled
    layer-1 depth 4 / 8 / 13 / 16 from both sides, 1 to 5 gW1 slots per wave, 3 / 6 / 9 / 12 gW3
    tiles over the eight waves."""
    fails = check_case(mode, S, A, rpb, N)
    assert not fails, fails


# ---- 3. nothing outside, nothing missing ----------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=P.MODE_NAMES)
@pytest.mark.parametrize("rpb,N", [(96, 200), (160, 330), (32, 549), (32, 1)])
def test_partials_written_exactly(mode, rpb, N):
    """launch() pre-fills [blocks][W] with NaN and a further block row with a sentinel: no NaN is
    left, the sentinel is untouched (EVAL: W = 2, so a pass that wrote [blocks][P] would hit it)."""
    part, _ = device_pass(mode, P.S1, P.A1, rpb, N)
    assert part.shape == ((N + rpb - 1) // rpb, 2 if mode == EVAL else P.param_count(P.S1, P.A1))
    assert np.isfinite(part).all()


@pytest.mark.parametrize("mode", MODES, ids=P.MODE_NAMES)
@pytest.mark.parametrize("S,A,rpb,N", [(197, 36, 96, 200), (197, 36, 32, 17), (16, 16, 96, 70), (255, 49, 64, 65)])
def test_padded_inputs_bit_identical(mode, S, A, rpb, N):
    """ldo = S + 3, lda = A + 5 with NaN in the padding columns and in 40 rows past N: the bits of
    the contiguous run (a read of a padding column or of a row past N would poison a sum)."""
    d, c = P.inputs(S, A, N), ctx_for(S, A)
    obs = torch.full((N + 40, S + 3), float("nan"), dtype=torch.float32, device=DEV)
    act = torch.full((N + 40, A + 5), float("nan"), dtype=torch.float32, device=DEV)
    obs[:N, :S] = to_dev(d["obs"])
    act[:N, :A] = to_dev(d["act"])
    adv = torch.full((N + 40,), float("nan"), dtype=torch.float64, device=DEV)
    adv[:N] = to_dev(d["adv"])
    part, _ = launch(c, mode, N, obs, act, adv, to_dev(d["theta"]), to_dev(P.mode_vec(d, mode)), rpb)
    np.testing.assert_array_equal(part, device_pass(mode, S, A, rpb, N)[0])


# ---- 4. exact cases -------------------------------------------------------------------------
@pytest.mark.parametrize("rpb,N", P.BLOCK_CASES)
def test_eval_at_new_equals_old_is_exact(rpb, N):
    """vec == theta: LR = exp(0) = 1 and every sample_kl term cancels, so with advantages k/64
    (exactly summable) each block's partial is (sum adv, 0.0) bit for bit."""
    d = P.inputs(P.S1, P.A1, N)
    part, red = device_pass(EVAL, P.S1, P.A1, rpb, N, exact=True)
    want = np.array([[d["adv_exact"][r0:r1].sum(), 0.0] for r0, r1 in P.block_ranges(rpb, N)])
    np.testing.assert_array_equal(part, want)
    assert not np.signbit(part[:, 1]).any()
    np.testing.assert_array_equal(red, [d["adv_exact"].sum(), 0.0])


@pytest.mark.parametrize("rpb,N", P.BLOCK_CASES)
def test_fvp_log_std_slots_are_zero(rpb, N):
    part, red = device_pass(FVP, P.S1, P.A1, rpb, N)
    for x in (part[:, -P.A1:], red[-P.A1:]):
        assert (x == 0.0).all() and not np.signbit(x).any()


@pytest.mark.parametrize("blocks", [1, 15, 16, 17, 32, 33, 257])
def test_reduce_exact_on_summable_partials(blocks):
    """amx_npg_reduce (one stage up to 16 blocks, two above) on integers / 64: the numpy column sum
    bit for bit, at widths around the 256-thread launch block and the flagship P."""
    c = ctx_for(P.S1, P.A1)
    rs = np.random.RandomState(blocks)
    for W in (1, 2, 255, 256, 257, P.param_count(P.S1, P.A1)):
        part = rs.randint(-2 ** 20, 2 ** 20 + 1, (blocks, W)) / 64.0
        np.testing.assert_array_equal(reduce(c, to_dev(part), blocks, W), part.sum(0))


# ---- 5. the pinned variants at multi-chunk blocks -------------------------------------------
N5 = 330


@pytest.fixture(scope="module", params=[96, 160])
def npg_mc(request):
    """DeviceNPG on the flagship shape with 3 / 5 chunks per block (N = 330: blocks of 96, 96, 96,
    42 rows or 160, 160, 10) and its device inputs."""
    import amp_extensions_amd as amx
    from amp_extensions_amd.npg import unpack_policy
    d = P.inputs(P.S1, P.A1, N5)
    layers, ls = unpack_policy(d["theta"], P.S1, P.A1)
    npg = amx.DeviceNPG(ctx_for(P.S1, P.A1), layers, ls, normalized_step_size=0.1,
                        FIM_invert_args={"iters": 3, "damping": 1e-4}, min_log_std=-2.0)
    rpb = request.param
    npg._rows_per_block = lambda n: rpb
    o, a, adv = npg._inputs(d["obs"], d["act"], d["adv"])
    return npg, d, o, a, adv, to_dev(d["vec"]), to_dev(d["new"])


def test_mc_theta_cache_bit_identical(npg_mc):
    from amp_extensions_amd.npg import NPG_FVP, NPG_VPG
    npg, d, o, a, adv, vec, _ = npg_mc
    hc = torch.full((N5, 64), float("nan"), dtype=torch.float32, device=DEV)
    v0 = npg._pass(NPG_VPG, o, a, adv, None, reduce=False).clone()
    v1 = npg._pass(NPG_VPG, o, a, adv, None, hcache=hc, reduce=False).clone()
    assert torch.equal(v0, v1) and not torch.isnan(hc).any()
    h0 = npg._pass(NPG_FVP, o, a, None, vec, reduce=False).clone()
    h1 = npg._pass(NPG_FVP, o, a, None, vec, hcache=hc, reduce=False).clone()
    assert torch.equal(h0, h1), float((h0 - h1).abs().max())


def _hcache_rows(npg_mc):
    from amp_extensions_amd.npg import NPG_VPG
    npg, d, o, a, adv, _, _ = npg_mc
    hc = torch.full((N5, 64), float("nan"), dtype=torch.float32, device=DEV)
    npg._pass(NPG_VPG, o, a, adv, None, hcache=hc)
    torch.cuda.synchronize()
    return hc.cpu().numpy()


def test_mc_hcache_within_4ulp_of_fp64_tanh(npg_mc):
    """The rows the VPG pass caches (H1 | H2) against the fp64 forward's tanh activations, within 4
    ulp of fp32.  The distance is absolute, not relative to the value -- it is the rounding of a
    197-term fp32 dot product under tanh' <= 1, plus tanhf's own -- so it is counted in fp32 ulps of
    tanh's top binade [0.5, 1), 2^-24.

    Observed on an MI355X, at 3 and at 5 chunks per block: H1 2.94 ulp, H2 2.21 ulp.  This test
    found layer 1's summation: as two fma chains of ~99 terms each it left H1 4.31 ulp away (4.22 of
    them the dot product's fp32 rounding at |z| = 0.54, before any tanhf -- the correctly rounded
    host evaluation of the same two chains gave the same 4.307382170110941); as four chains of ~50
    the host evaluation gives 3.01 and the device 2.94."""
    _, d = npg_mc[:2]
    h1r, h2r, _ = P._forward(P.unpack(d["theta"], P.S1, P.A1), d["obs"].astype(np.float64))
    dist = np.abs(_hcache_rows(npg_mc).astype(np.float64) - np.concatenate([h1r, h2r], 1)) / 2.0 ** -24
    print(f"HCACHE vs fp64 forward: H1 {dist[:, :32].max():.2f} H2 {dist[:, 32:].max():.2f} ulp (2^-24)")
    assert dist.max() <= 4.0, dist.max()


def test_mc_hcache_is_tanh_of_the_kernels_sums(npg_mc):
    """The cached rows against the fp64 tanh of the kernel's own fp32 pre-activations, restated on
    the host in the kernel's order (layer 1: four fma chains, ((c0 + c2) + (c1 + c3)) + b1;
    layer 2: one fma chain over the CACHED H1 row, + b2): within 4 ulp of the value itself, so
    every cached element is the activation of its own row and unit, and the device tanhf is good
    to 4 ulp (its documented bound is 2; one more for an MFMA sum that rounds differently from the
    host's fma)."""
    _, d = npg_mc[:2]
    hc = _hcache_rows(npg_mc)
    want = np.concatenate([P.kernel_h1(d["theta"], d["obs"], P.S1, P.A1),
                           P.kernel_h2(d["theta"], hc[:, :32], P.S1, P.A1)], 1)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    dist = np.abs(hc.astype(np.float64) - want) / ulp
    print(f"HCACHE vs tanh of the kernel's sums: H1 {dist[:, :32].max():.2f} H2 {dist[:, 32:].max():.2f} ulp of the value")
    assert dist.max() <= 4.0, dist.max()


@pytest.mark.parametrize("M", [70, 200])
def test_mc_indexed_rows_bit_identical(npg_mc, M):
    """Index vector with duplicates and a reversed run; with the theta cache and without."""
    from amp_extensions_amd.npg import NPG_FVP, NPG_VPG
    npg, _, o, a, adv, vec, _ = npg_mc
    rs = np.random.RandomState(M)
    idx = rs.randint(0, N5, M)
    idx[5:25] = np.arange(N5 - 1, N5 - 21, -1)   # a reversed run ending at the last row
    idx[30:34] = idx[29]                         # duplicates
    idx_t = torch.from_numpy(idx.astype(np.int32)).to(DEV)
    rows = o[idx_t.long()].contiguous()
    plain = npg._pass(NPG_FVP, rows, a[:M], None, vec, reduce=False).clone()
    assert torch.equal(npg._pass_idx(o, idx_t, vec).clone(), plain)
    hc = npg._hcache(N5)
    npg._pass(NPG_VPG, o, a, adv, None, hcache=hc)
    assert torch.equal(npg._pass_idx(o, idx_t, vec, hcache=hc).clone(), plain)


def test_mc_input_dtypes_bit_identical(npg_mc):
    """fp64 / fp64 inputs and the two mixed kernels (f64 obs with f32 act, f32 obs with f64 act; FVP
    reads no actions) give the f32 / f32 bits."""
    npg, _, o, a, adv, vec, new = npg_mc
    o64, a64 = o.double(), a.double()
    for mode, v in ((VPG, None), (FVP, vec), (EVAL, new)):
        base = npg._pass(mode, o, a, adv, v, reduce=False).clone()
        for oo, aa in ((o64, a64), (o64, a), (o, a64)):
            assert torch.equal(npg._pass(mode, oo, aa, adv, v, reduce=False), base), (mode, oo.dtype, aa.dtype)


def test_mc_cg_fold_bit_identical(npg_mc):
    """3 iterations of cg_solve with the vector step folded into the next pass against the unfolded
    form, with the theta cache."""
    from amp_extensions_amd.npg import NPG_VPG
    npg, _, o, a, adv, _, _ = npg_mc
    hc = npg._hcache(N5)
    b = npg._pass(NPG_VPG, o, a, adv, None, hcache=hc).clone()
    xs = []
    for fold in (False, True):
        npg.cg_fold, npg.residual_tol = fold, 0.0
        xs.append(npg.cg_solve(o, a, b, hcache=hc).clone())
    npg.cg_fold = True
    assert torch.isfinite(xs[0]).all() and float(xs[0].abs().max()) > 0
    assert torch.equal(xs[0], xs[1]), float((xs[0] - xs[1]).abs().max())


# ---- 6. DeviceNPG.surrogate_kl --------------------------------------------------------------
def test_surrogate_kl_vs_reference():
    import amp_extensions_amd as amx
    from amp_extensions_amd.npg import unpack_policy
    S, A, N = P.S1, P.A1, 200
    d = P.inputs(S, A, N)
    layers, ls = unpack_policy(d["theta"], S, A)
    npg = amx.DeviceNPG(ctx_for(S, A), layers, ls)
    o, a, adv = npg._inputs(d["obs"], d["act"], d["adv"])
    surr, kl = npg.surrogate_kl(o, a, adv, to_dev(d["new"]))
    ref, mag = P.pass_ref(EVAL, S, A, d["theta"], d["obs"], d["act"], d["adv"], d["new"])
    r = P.ratio([surr * N, kl * N], ref, mag)
    print(f"SURROGATE_KL ratios surr {r[0]:.3f} kl {r[1]:.3f}")
    assert (r <= P.allowance(EVAL, N)).all(), r
