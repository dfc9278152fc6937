"""The returns / baseline-feature / value-head / GAE / whitening kernels (csrc/amx_gae.hip) through
the C ABI against the plain per-trajectory reference (tests/gae_ref.py, pinned on the CPU by
test_cpu_gae_ref.py), at the shapes and values where they can go wrong.  Every buffer a kernel
writes starts as NaN, everything it must not read holds NaN, everything it must not write is
checked afterwards.

Exact (bits; NaN where the reference has NaN): the features at every S around the K tile and the
wave, padded leading dimensions, ragged lanes, t0 with ends mid-lane, the clip's edges, subnormal
results and positions past 5000; returns and advantages in both modes and both delta precisions at
L around the 256-thread block, every end pattern, separate reward layouts and a NaN fence; the head
on exactly summable operands.
Bounded: the head on generic operands, |v - ref| <= 2^-24 |s| + 2^-24 |v| + 70 * 2^-53 * mag
(test_head); the whitening, at gae_cases.ALLOW = 4 / 4 / 16 x numpy's own measured error (elem 12.4,
mean 6.8, sd 62.4 in the units of gae_cases; test_cpu_gae_ref.py::test_whitening_yardstick).
"""
import numpy as np
import pytest
import torch

import gae_cases as C
import gae_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
_CTX = {}


def ctx_for(S):
    import amp_extensions_amd as amx
    if S not in _CTX:
        _CTX[S] = amx.AmxContext(S, 4, n_models=1, hidden=128, n_hidden=1, device=DEV)
    return _CTX[S]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(c, rc):
    assert rc == 0, c.lib.amx_last_error().decode()
    torch.cuda.synchronize()


def assert_bits(got, exp, what=""):
    """Same NaN positions, same bits everywhere else (so -0.0 is not 0.0)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    ng, ne = np.isnan(got), np.isnan(exp)
    np.testing.assert_array_equal(ng, ne, err_msg=f"{what}: NaN positions")
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = (got.view(u) != exp.view(u)) & ~ne
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]!r} != {exp[bad][0]!r}"


# ---- features ----------------------------------------------------------------------------------
def special_values():
    ten = np.float64(10.0)
    return np.array([10.0, -10.0, np.nextafter(ten, np.inf), np.nextafter(-ten, -np.inf), np.nextafter(ten, 0.0),
                     np.nextafter(-ten, 0.0), np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-39, 5e-45 * 10, -1e-39,
                     1e300, -1e300])


def observations(nrows, S, ldo, seed):
    """[nrows, ldo] float64: entry (r, j) cycles through the special values (the clip's edges and
    their neighbours, +-inf, NaN, +-0, values whose tenth is subnormal in float32, +-1e300) and
    ordinary ones (a third of the entries, N(0, 6^2): some clipped); columns past S hold NaN."""
    sp = special_values()
    rs = np.random.RandomState(seed)
    o = rs.randn(nrows, ldo) * 6.0
    k = (np.arange(nrows)[:, None] * 5 + np.arange(ldo)[None, :] * 7) % 24
    o = np.where(k < len(sp), sp[np.minimum(k, len(sp) - 1)], o)
    o[:, S:] = np.nan
    return o


def feature_grid(L, layout, t0_mode, seed):
    """A small grid of L lanes of up to T = 6 rows.  layout 'paths': concatenated paths (base =
    offsets with a gap of one unowned row after each path, stride 1, ragged len incl. 0 and T);
    'lanes': [T, L] with stride L (ragged len for odd L, none for even).  Lane 0 is full length and
    ends a trajectory at its third row; in the 'mixed' mode its t0 is 4000."""
    rs = np.random.RandomState(seed)
    T = 6
    len_ = rs.randint(0, T + 1, size=L)
    len_[0] = T
    if L > 1:
        len_[1] = 0
    if L > 2:
        len_[2] = T
    if layout == "paths":
        base = np.concatenate([[0], np.cumsum(len_ + 1)[:-1]]).astype(np.int64)
        stride, nrows = 1, int((len_ + 1).sum())
    else:
        base, stride, nrows = None, L, T * L
        if L % 2 == 0:
            len_ = None
    end = rs.choice([0, 0, 0, 1, 2], size=nrows).astype(np.uint8)
    r0 = 0 if base is None else int(base[0])
    end[[r0, r0 + stride, r0 + 2 * stride]] = [0, 0, 1]
    t0 = {"none": None, "zeros": np.zeros(L, np.int32),
          "mixed": rs.choice([0, 1, 999, 1000, 4000], size=L).astype(np.int32)}[t0_mode]
    if t0_mode == "mixed":
        t0[0] = 4000
    return dict(T=T, L=L, len=None if len_ is None else len_.astype(np.int32), base=base, stride=stride, end=end,
                t0=t0, nrows=nrows)


def run_features(S, g, ldo, ldf_pad, seed):
    c = ctx_for(S)
    kf = (S + 4 + 31) // 32 * 32
    ldf = kf + ldf_pad
    obs = observations(g["nrows"], S, ldo, seed)
    feat = torch.full((g["nrows"], ldf), float("nan"), dtype=torch.float32, device=DEV)
    keep = [dev(g[k]) for k in ("len", "t0", "base")] + [dev(g["end"]), dev(obs)]
    ok(c, c.lib.amx_value_features(c.h, g["T"], g["L"], ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), g["stride"],
                                   keep[3].data_ptr(), keep[4].data_ptr(), ldo, feat.data_ptr(), ldf, c.stream))
    exp = np.full((g["nrows"], ldf), np.nan, dtype=f32)
    for rows, _, pos in G.split(g["T"], g["L"], g["len"], g["base"], g["stride"], g["end"], g["t0"]):
        exp[rows, :kf] = G.features(obs[rows], S, kf, pos + np.arange(len(rows)))
    return feat.cpu().numpy(), exp, kf


@pytest.mark.parametrize("S", [1, 27, 28, 29, 60, 63, 64, 65, 124, 197, 226])
def test_features_bit_exact(S):
    """S + 4 on, just before and just past a 32-column K tile, S below / at / above one wave's 64
    lanes, and the two production widths; per S every L in {1, 3, 4, 5, 9} x both layouts x t0 in
    {none, zeros, mixed with 4000 on a lane that ends a trajectory mid-lane}, the four (ldo, ldf)
    = (S | S + 3, kf | kf + 96) taken in turn (each at least seven times per S).  Rows outside the
    grid and columns past kf keep their NaN; columns S+4 .. kf-1 are written as zero."""
    i, seen = 0, set()
    for L in (1, 3, 4, 5, 9):
        for layout in ("paths", "lanes"):
            for t0_mode in ("none", "zeros", "mixed"):
                g = feature_grid(L, layout, t0_mode, seed=100 * L + i)
                ldo, pad = S + 3 * (i % 2), 96 * ((i // 2) % 2)
                got, exp, kf = run_features(S, g, ldo, pad, seed=i)
                assert_bits(got, exp, f"S={S} L={L} {layout} t0={t0_mode} ldo={ldo} ldf=kf+{pad}")
                if t0_mode == "mixed":  # the lane with t0 = 4000 restarts at 0 after its end flag
                    r3 = (0 if g["base"] is None else g["base"][0]) + 3 * g["stride"]
                    assert got[r3, S] == 0.0 and got[r3 - g["stride"], S] == f32(4.002)
                seen.add((ldo - S, pad))
                i += 1
    assert seen == {(0, 0), (3, 0), (0, 96), (3, 96)}


def test_features_long_lane_positions_past_5000():
    """One lane of 1100 rows from t0 = 4000 with an end at row 1050: positions 4000 .. 5050 (al > 1
    from 1001 on, so pow's 3rd and 4th powers grow), then 0 .. 48."""
    S = 28
    end = np.zeros(1100, np.uint8)
    end[1050] = 1
    g = dict(T=1100, L=1, len=np.array([1100], np.int32), base=np.array([0], np.int64), stride=1, end=end,
             t0=np.array([4000], np.int32), nrows=1100)
    got, exp, kf = run_features(S, g, S, 0, seed=3)
    assert_bits(got, exp, "long lane")
    assert got[1050, S] == f32(5.05) and got[1050, S + 3] == f32(5.05 ** 4) and got[1051, S] == 0.0


def test_features_subnormal_and_clip_values():
    """The special values themselves, one per column at S = 29 (16 of them, twice: the second half
    of the row repeats the first, minus the last three): a tenth of 1e-39 and of 5e-44 are
    subnormal float32 numbers (not flushed), -0.0 keeps its sign, the neighbours of +-10 inside the
    clip round to +-1, NaN passes."""
    S = 29
    c = ctx_for(S)
    sp = special_values()
    obs = np.concatenate([sp, sp[:13]])[None, :]
    feat = torch.full((1, 96), float("nan"), dtype=torch.float32, device=DEV)
    end, o = dev(np.zeros(1, np.uint8)), dev(obs)
    ok(c, c.lib.amx_value_features(c.h, 1, 1, None, None, None, 1, end.data_ptr(), o.data_ptr(), S, feat.data_ptr(), 96,
                                   c.stream))
    got = feat.cpu().numpy()
    assert_bits(got[:, :64], G.features(obs, S, 64, np.arange(1)), "specials")
    assert np.isnan(got[:, 64:]).all()
    with np.errstate(all="ignore"):
        hand = (np.array([10, -10, 10, -10, np.nextafter(10.0, 0), np.nextafter(-10.0, 0), 10, -10, np.nan, 0.0, -0.0,
                          1e-39, 5e-44, -1e-39, 10, -10]) / 10.0).astype(f32)
    assert_bits(got[0, :16], hand, "specials by hand")
    assert 0 < got[0, 11] < np.finfo(f32).tiny and got[0, 12] == f32(4 * 2.0 ** -149) and np.signbit(got[0, 10])


# ---- head --------------------------------------------------------------------------------------
def head_inputs(kind, rows, H, seed):
    rs = np.random.RandomState(seed)
    if kind == "exact":  # |integers| <= 4 times 2^-2..2: any sum of <= 256 products is a multiple of 2^-4 below 2^16
        h = (rs.randint(-4, 5, size=(rows, H)) * 2.0 ** rs.randint(-2, 3, size=(rows, H))).astype(f32)
        w = (rs.randint(-4, 5, size=H) * 2.0 ** rs.randint(-2, 3, size=H)).astype(f32)
        return h, w, f32(0.375)
    h, w = rs.randn(rows, H).astype(f32), rs.randn(H).astype(f32)
    if rows and H > 1:  # row 0 cancels: its last term undoes the others up to float32 rounding
        h[0] *= 1e3
        h[0, -1] = f32(-(h[0, :-1].astype(np.float64) @ w[:-1].astype(np.float64)) / w[-1])
    return h, w, f32(rs.randn())


@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 127, 128, 200, 256])
def test_head(H):
    """Linear(H -> 1) at H below, at and off the 64-lane stride, rows in {0, 1, 3, 4, 5, 130} (four
    rows per workgroup), ldh = H and H + 7 (NaN in the padding, after w's H entries and in v past
    `rows`).

    exact: every partial sum in any order is exact in float64 and the result in float32, so the
    device equals gae_ref.head bit for bit.
    generic (randn; row 0 cancels to ~1e-8 of its magnitude): the device adds at most 64 strided
    terms per lane and 6 butterfly steps in float64, each rounding at most 2^-53 of a partial sum
    of magnitude <= mag = sum |h_k w_k|: |s_dev - s| <= 70 * 2^-53 * mag.  Rounding s to float32
    costs at most 2^-24 |s| and the float32 add of b at most 2^-24 |v|:
        |v - ref| <= 2^-24 |s| + 2^-24 |v| + 70 * 2^-53 * mag.
    (Two float32 roundings of sums 70 * 2^-53 * mag apart can differ by a whole ulp, up to
    2^-23 |s|; on these inputs that needs s within ~1e-14 mag of a rounding boundary, or the
    cancelling row, where the last term dominates the bound anyway.)
    Measured on an MI355X: every generic row equals the reference too (largest |v - ref| / bound 0)."""
    c = ctx_for(28)
    worst = 0.0
    for rows in (0, 1, 3, 4, 5, 130):
        for ldh in (H, H + 7):
            for kind in ("exact", "generic"):
                h, w, b = head_inputs(kind, rows, H, seed=rows * 31 + ldh)
                hb = np.full((max(rows, 1), ldh), np.nan, dtype=f32)
                hb[:rows, :H] = h
                wb = np.full(H + 8, np.nan, dtype=f32)
                wb[:H] = w
                hd, wd, bd = dev(hb), dev(wb), dev(np.array([b, np.nan], f32))
                v = torch.full((rows + 4,), float("nan"), dtype=torch.float32, device=DEV)
                ok(c, c.lib.amx_value_head(c.h, rows, hd.data_ptr(), ldh, H, wd.data_ptr(), bd.data_ptr(), v.data_ptr(),
                                           c.stream))
                got = v.cpu().numpy()
                assert np.isnan(got[rows:]).all(), "the head wrote past `rows`"
                ref = [G.head(h[r], w, b) for r in range(rows)]
                if kind == "exact":
                    assert_bits(got[:rows], np.array([r[0] for r in ref], dtype=f32), f"H={H} rows={rows} ldh={ldh}")
                    continue
                for r, (rv, s, mag) in enumerate(ref):
                    bound = 2.0 ** -24 * abs(s) + 2.0 ** -24 * abs(float(got[r])) + 70 * 2.0 ** -53 * mag
                    err = abs(float(got[r]) - float(rv))
                    worst = max(worst, err / bound)
                    assert err <= bound, (H, rows, ldh, r, got[r], rv, err, bound)
    print(f"HEAD H={H}: largest |v - ref| / bound = {worst:.3f}")


# ---- returns and advantages --------------------------------------------------------------------
def gae_grids():
    """(name, T, L, len, base, stride): [T, L] lane buffers at L around the 256-thread block (the
    stride padded by 3 at T = 2), and one ragged concatenated-paths grid with gaps between paths."""
    out = [(f"L{L}xT{T}", T, L, None, None, L + (3 if T == 2 else 0)) for L in (1, 255, 256, 257) for T in (1, 2, 7)]
    len_ = np.array([0, 1, 2, 33, 1, 0, 33, 2], np.int32)
    base = np.concatenate([[0], np.cumsum(len_ + 2)[:-1]]).astype(np.int64)
    out.append(("ragged", 33, len(len_), len_, base, 1))
    return out


def run_gae(c, T, L, len_, base, stride, end, rew_rows, v_rows, nrows, gamma, lam, rlayout):
    """amx_gae on a grid whose row space [nrows] holds NaN (v), 1 (end) outside the grid; the
    rewards lie like the grid ('same') or in their own [T, L + 5] buffer ('own').  -> ret, adv over
    the row space (NaN-filled before the launch)."""
    from amp_extensions_amd.gae import gamma_lambda
    rows, cells = C.grid_rows(T, L, len_, base, stride)
    vb = np.full(nrows, np.nan, dtype=f32)
    vb[rows] = v_rows[rows]
    eb = np.ones(nrows, dtype=np.uint8)
    eb[rows] = end[rows]
    if rlayout == "same":
        rb = np.full(nrows, np.nan, dtype=f32)
        rb[rows] = rew_rows[rows]
        rbase, rstride = base, stride
    else:
        Lp = L + 5
        rb = np.full(T * Lp + nrows, np.nan, dtype=f32)  # a NaN tail as long as the row space
        rb[(cells // L) * Lp + cells % L] = rew_rows[rows]
        rbase, rstride = None, Lp
    ret = torch.full((nrows + 8,), float("nan"), dtype=torch.float64, device=DEV)
    adv = torch.full((nrows + 8,), float("nan"), dtype=torch.float64, device=DEV)
    keep = [dev(len_), dev(base), dev(eb), dev(rb), dev(rbase), dev(vb)]
    ok(c, c.lib.amx_gae(c.h, T, L, ptr(keep[0]), ptr(keep[1]), stride, keep[2].data_ptr(), keep[3].data_ptr(),
                        ptr(keep[4]), rstride, keep[5].data_ptr(), float(gamma), gamma_lambda(gamma, lam),
                        ret.data_ptr(), adv.data_ptr(), c.stream))
    return ret.cpu().numpy(), adv.cpu().numpy()


def gae_reference(T, L, len_, base, stride, end, rew_rows, v_rows, nrows, gamma, lam):
    ret, adv = np.full(nrows + 8, np.nan), np.full(nrows + 8, np.nan)
    for rows, term, _ in G.split(T, L, len_, base, stride, end, None):
        ret[rows] = G.returns(rew_rows[rows], gamma)
        adv[rows] = G.advantages(rew_rows[rows], v_rows[rows], term, gamma, lam)
    return ret, adv


@pytest.mark.parametrize("grid", gae_grids(), ids=lambda g: g[0])
def test_returns_and_advantages_bit_exact(grid):
    """Every end pattern (none: every lane cut; every row; last row only; random at p = 0.3; value
    2 mid-lane) x every (gamma, lambda) of gae_cases.GAMMA_LAMBDA (gamma 0 and 1, lambda 0 -- GAE
    mode with gl = 0 -- and 1, the three standard-mode spellings) x rewards laid like the grid and
    in a [T, L + 5] buffer of their own.  Rows outside the grid (len < T, the gaps of a padded
    stride or between paths) and the 8 doubles past the row space keep their NaN.  The values are
    gae_cases.gae_values (seed 0), on which test_cpu_gae_ref.py shows that the other delta
    precision or a fused multiply-add would change advantages."""
    name, T, L, len_, base, stride = grid
    c = ctx_for(28)
    rows, _ = C.grid_rows(T, L, len_, base, stride)
    nrows = int(rows.max()) + 1 + (2 if base is not None else 0)
    rew, v = C.gae_values(nrows, 0)
    for pattern in C.END_PATTERNS:
        end = C.end_flags(pattern, T, L, len_, base, stride, nrows)
        for gamma, lam in C.GAMMA_LAMBDA:
            exp_ret, exp_adv = gae_reference(T, L, len_, base, stride, end, rew, v, nrows, gamma, lam)
            for rlayout in ("same", "own"):
                ret, adv = run_gae(c, T, L, len_, base, stride, end, rew, v, nrows, gamma, lam, rlayout)
                what = f"{name} end={pattern} gamma={gamma} lambda={lam} rewards={rlayout}"
                assert_bits(ret, exp_ret, "returns " + what)
                assert_bits(adv, exp_adv, "advantages " + what)


@pytest.mark.parametrize("lam", [0.97, None])
def test_gae_fence_at_trajectory_ends(lam):
    """Three lanes of nine rows; lane 1 holds three trajectories (end 1 after row 2, end 2 after
    row 5), the middle one with a NaN reward and an inf value.  Its neighbours in the lane (and the
    other lanes) equal the reference bit for bit and are finite; the middle one is NaN exactly
    where numpy's is."""
    T, L = 9, 3
    c = ctx_for(28)
    end = np.zeros(T * L, np.uint8)
    end[2 * L + 1], end[5 * L + 1] = 1, 2
    rew, v = C.gae_values(T * L, 7)
    rew[4 * L + 1], v[5 * L + 1] = np.nan, np.inf
    exp_ret, exp_adv = gae_reference(T, L, None, None, L, end, rew, v, T * L, 0.995, lam)
    ret, adv = run_gae(c, T, L, None, None, L, end, rew, v, T * L, 0.995, lam, "same")
    assert_bits(ret, exp_ret, "returns")
    assert_bits(adv, exp_adv, "advantages")
    mid = np.arange(3, 6) * L + 1
    outer = np.setdiff1d(np.arange(T * L), mid)
    assert np.isfinite(ret[outer]).all() and np.isfinite(adv[outer]).all()
    assert np.isnan(ret[mid[:2]]).all() and not np.isnan(ret[mid[2]]) and not np.isfinite(adv[mid]).all()


# ---- whitening ---------------------------------------------------------------------------------
def run_whiten(c, case, in_place):
    x = dev(case["buf"])
    out = x if in_place else torch.full_like(x, float("nan"))
    stats = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    keep = [dev(case["len"]), dev(case["base"])]
    ok(c, c.lib.amx_adv_whiten(c.h, case["T"], case["L"], ptr(keep[0]), ptr(keep[1]), case["stride"], x.data_ptr(),
                               C.EPS, out.data_ptr(), stats.data_ptr(), c.stream))
    st = stats.cpu().numpy()
    assert np.isnan(st[2])
    return out.cpu().numpy(), st[:2]


@pytest.mark.parametrize("case", C.whiten_cases(), ids=lambda c: c["name"])
def test_whitening(case):
    """amx_adv_whiten on every input of gae_cases.whiten_cases against gae_ref.whiten (more than
    float64) within gae_cases.ALLOW, the allowance derived on the CPU from numpy's own error; run
    twice out of place (same bits: deterministic) and once in place (same bits again); cells outside
    the grid hold NaN on input and are NaN afterwards; an empty grid gives stats [0, 0] and writes
    no output; constant input gives exactly 0 and [0.75, 0].

    Measured on an MI355X, the largest error over the cases (numpy's in brackets, allowance after):
    elem 3.68 at flat8193 (3.04; 12.4), mean 1.54 at engine9x257+31 (1.66; 6.8), sd 3.86 at ill1e6
    (3.86; 62.4); process_samples 2.04 / 1.27 per element.  With the kernel as it was before these
    tests (Chan's combine about each chunk's rounded mean, the mean as sum / n) the ill-conditioned
    inputs fail: sd off by 1.9e6 (ill1e6), 4.7e5 (ill-3e8) and 6.1e4 (leadempty) units on the MI355X."""
    c = ctx_for(28)
    out, st = run_whiten(c, case, False)
    out2, st2 = run_whiten(c, case, False)
    out3, st3 = run_whiten(c, case, True)
    rows = case["rows"]
    gaps = np.setdiff1d(np.arange(len(case["buf"])), rows)
    assert np.isnan(out[gaps]).all() and np.isnan(out3[gaps]).all(), "a cell outside the grid was written"
    assert_bits(out2, out, "second run")
    assert_bits(out3, out, "in place")
    assert_bits(st2, st, "stats, second run")
    assert_bits(st3, st, "stats, in place")
    x = case["buf"][rows]
    if x.size == 0:
        assert st.tolist() == [0.0, 0.0]
        return
    assert not np.isnan(out[rows]).any()
    ref_out, ref_mean, ref_sd = G.whiten(x, C.EPS)
    e = C.whiten_errors(x, out[rows], st[0], st[1], ref_out, ref_mean, ref_sd, C.EPS)
    print(f"WHITEN device {case['name']}: elem {e[0]:.2f} mean {e[1]:.2f} sd {e[2]:.2f}")
    if case["name"] == "const":
        assert not out[rows].any() and st.tolist() == [0.75, 0.0]
    assert e[0] <= C.ALLOW["elem"] and e[1] <= C.ALLOW["mean"] and e[2] <= C.ALLOW["sd"], (e, C.ALLOW)


# ---- process_samples ---------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.97, None])
def test_process_samples_normalize(lam):
    """process_samples(..., normalize=True) (utils/process_samples.py:14-19 / 30-35, eps 1e-8) on six
    short paths at S = 28, one of a single row, terminated and not: returns bit for bit; the
    advantages are gae_ref's on the device's own baseline values, whitened, within the whitening
    allowance per element; dtypes float64 / float32 / float64; the returned tensors are the path
    entries.  The rewards are 1 + 0.3 N(0, 1), so the advantages' mean is of their own size (the
    element unit 2^-53 (|x| + |mean|) / sd then bounds the mean's error too)."""
    import amp_extensions_amd as amx
    from oracle import milo_ref as R
    S, gamma = 28, 0.995
    c = ctx_for(S)
    rs = np.random.RandomState(4)
    paths = []
    for i, l in enumerate([9, 1, 17, 4, 30, 12]):
        paths.append(dict(observations=rs.randn(l, S) * 4.0, rewards=(1.0 + 0.3 * rs.randn(l)).astype(f32),
                          terminated=bool(i % 2)))
    layers = R.init_mlp_baseline(S, (128, 128), seed=9)
    bl = amx.DeviceMLPBaseline(c, layers)
    ret, adv, v = amx.process_samples(paths, bl, gamma, lam, normalize=True)
    torch.cuda.synchronize()
    assert (ret.dtype, adv.dtype, v.dtype) == (torch.float64, torch.float64, torch.float32)
    assert_bits(ret.cpu().numpy(), np.concatenate([p["returns"] for p in paths]), "returned returns")
    assert_bits(adv.cpu().numpy(), np.concatenate([p["advantages"] for p in paths]), "returned advantages")
    assert_bits(v.cpu().numpy(), np.concatenate([p["baseline"] for p in paths]), "returned values")
    raw = []
    for p in paths:
        assert (p["returns"].dtype, p["baseline"].dtype, p["advantages"].dtype) == (np.float64, f32, np.float64)
        assert_bits(p["returns"], G.returns(p["rewards"], gamma), "returns")
        raw.append(G.advantages(p["rewards"], p["baseline"], p["terminated"], gamma, lam))
    feat = np.concatenate([G.features(p["observations"], S, S + 4, np.arange(len(p["rewards"]))) for p in paths])
    np.testing.assert_allclose(v.cpu().numpy(), R.mlp_baseline_predict(layers, feat), rtol=2e-5, atol=1e-6)
    raw = np.concatenate(raw)
    ref_out, ref_mean, ref_sd = G.whiten(raw, 1e-8)
    got = adv.cpu().numpy()
    e = C.whiten_errors(raw, got, ref_mean, ref_sd, ref_out, ref_mean, ref_sd, 1e-8)
    print(f"WHITEN device process_samples lambda={lam}: elem {e[0]:.2f}")
    assert e[0] <= C.ALLOW["elem"], e
