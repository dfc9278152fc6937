"""Exactly summable operands for the ensemble GEMM, a numpy restatement of the f16x3 algorithm
 and the table of shapes that reach each tile family (numpy only: importable
without a GPU).

The f16x3 GEMM writes a fp32 operand row as 2^(E-14) (hi + lo) with two fp16 limbs and sums
hi*hi' + hi*lo' + lo*hi' in fp32 on the matrix pipe.  fp32 addition is exact whenever every
partial sum is a multiple of a common granule g and stays below 2^24 g, whatever the order of
the additions.  The two builders below produce operands whose limbs are known in closed form
and for which

    max over outputs of sum_k (|hi||hi'| + |hi||lo'| + |lo||hi'|)  <  2^22 g

(two bits below fp32's 24, so exactness does not rest on how an MFMA aligns its internal
adds).  For such operands every tile family, every K split and every stream-K combine order
must produce the same bits, and those bits are the ones the restatement computes in fp64: the
GPU tests compare with np.array_equal, no tolerance.

  tier 1 (one limb)   integers |v| <= 15 times a per-row power of two: lo = 0; the same data
                      is exact for the bf16x6 tiles (8-bit limbs) and the f32 tiles.  Dense,
                      so every k of every tile contributes to every output.
  tier 2 (two limbs)  in the row's scaled units [2^13, 2^14) every nonzero is 1024 p + q/4
                      (p in +-{1..7}, q = +-1) beside one anchor of 8192 per row that fixes the
                      row exponent: hi = 1024 p, lo = q/4, neither rounding a tie (p = +-1
                      takes q of p's sign: 1023.75 would be a tie of the [512, 1024) binade).
                      A rows are dense; a W row has 12 nonzeros and the anchor.  g = 2^8 (the
                      cross products 1024 p * q/4), the sum is at most 13 * 2^26 < 2^30.

The groups of an A operand share their first 32 columns when a launch uses k_shared (member
0's are read for every member), so a row of A takes the same 2^r in every group and, in tier
2, its anchor lies past those columns: the operand the launch sees still has one scale and
one anchor per row.  The 12 nonzeros of the tier-2 W rows of a column tile touch every k when
the tile is at least 64 columns wide at K <= 352 (224 at K = 2304); the narrower stream-K tiles
get their every-k check from the dense tier 1.

pick_tile() restates the launchers' tile selection so the table can name the family each
shape reaches; it is a copy of branches in csrc/amx_gemm.hip and drifts if they change without
it -- the GPU tests only use it to label cases, the CPU test pins the table against it.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

HSC = 14          # scaled operands lie in [2^13, 2^14) (amx_h3.h)
N_CUS = 256       # the table is derived for the MI355X
MAX_ROWS = 8192   # most rows of any case; the 2304-deep cases stop at 6144
SHARED = 32       # k_shared of the cases that use one
A_DIM = 36        # action width of the test contexts (the GEMM entries do not read it)


# ---- the algorithm, restated ------------------------------------------------------------------
def row_exponent(x):
    """E with max|row| < 2^E (frexp exponent of the row maximum; -100 for a zero row), clamped
    to [-100, 100] as exp_of_bits does."""
    x = np.asarray(x)
    m = np.abs(x).max(axis=-1).astype(np.float64) if x.size else np.zeros(x.shape[:-1])
    e = np.where(m > 0, np.frexp(m)[1], -100)
    return np.clip(e, -100, 100).astype(np.int64)


def split_limbs(x, E):
    """(hi, lo) in fp64 of rows x scaled by 2^(14 - E): hi = RN_f16(xs), lo = RN_f16(xs - hi)."""
    xs = np.ldexp(np.asarray(x, np.float64), (HSC - np.asarray(E))[..., None]).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def h3_acc(A, W):
    """The three-product value acc = hi hi' + hi lo' + lo hi' (fp64, scaled units) of one group,
    with the exponents of the A rows and W rows."""
    Er, Ec = row_exponent(A), row_exponent(W)
    ah, al = split_limbs(A, Er)
    wh, wl = split_limbs(W, Ec)
    return ah @ (wh + wl).T + al @ wh.T, Er, Ec


def _to_f32_exact(v):
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "accumulator is not a fp32 value: operands are not exact"
    return out


def pre_bias(A, W, path):
    """fp32 [rows][N] value ahead of the bias for one group: the f16x3 accumulator un-scaled by
    2^(Er + Ec - 28), or A W^T itself on the f32 / bf16x6 paths (exact on tier-1 operands)."""
    if path == "h3":
        acc, Er, Ec = h3_acc(A, W)
        return _to_f32_exact(np.ldexp(acc, Er[:, None] + Ec[None, :] - 2 * HSC))
    return _to_f32_exact(np.asarray(A, np.float64) @ np.asarray(W, np.float64).T)


def hidden_epilogue(pre, bias):
    """ReLU(pre + bias) in fp32 and the row-exponent output of the N columns."""
    v = pre + bias.astype(np.float32)[None, :]
    v = np.where(v < 0, np.float32(0), v).astype(np.float32)
    return v, row_exponent(v)


def output_epilogue(pre, bias, sd_d, mu_d):
    """((pre + bias) * sd_d) + mu_d, one fp32 rounding per operation."""
    y = (pre + bias.astype(np.float32)[None, :]).astype(np.float32)
    prod = (y * sd_d.astype(np.float32)[None, :]).astype(np.float32)
    return (prod + mu_d.astype(np.float32)[None, :]).astype(np.float32)


# ---- exactness condition ------------------------------------------------------------------------
def granule(x):
    """Per row, the largest power of two dividing every nonzero element (inf for a zero row)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (M & -M).astype(np.float64)
    g = np.where(x != 0, np.ldexp(low, e - 53), np.inf)
    return g.min(axis=-1)


def _pair_granule(gah, gal, gwh, gwl):
    g = np.minimum(np.minimum(gah[:, None] * gwh[None, :], gah[:, None] * gwl[None, :]),
                   gal[:, None] * gwh[None, :])
    return np.where(np.isfinite(g), g, 1.0)  # a zero row: every term is zero


def _granule32(x):
    """granule() of a float32 array of normal numbers and zeros, on its bits."""
    b = x.view(np.uint32)
    e = ((b >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32)
    m = ((b & np.uint32(0x7fffff)) | np.uint32(0x800000)).astype(np.int32)
    g = np.where(e > 0, np.ldexp((m & -m).astype(np.float32), e - 150), np.float32(np.inf))
    return g.min(axis=-1).astype(np.float64)


def _rn_f16(x):
    """RN_f16 of a float32 array as float32, on its bits (numpy's own fp16 conversion takes
    seconds on the 50 M elements of a deep case); None when a value lies outside fp16's normal
    range, where the bit trick does not hold."""
    a = np.abs(x)
    if ((a != 0) & ((a < 2.0 ** -14) | (a >= 65504.0))).any():
        return None
    b = x.view(np.uint32)
    r = (b + np.uint32(0xfff) + ((b >> np.uint32(13)) & np.uint32(1))) & np.uint32(0xffffe000)
    return r.view(np.float32)


def row_stats(x):
    """Per row of one group's operand: (max|hi|, max|lo|, sum|hi|, sum|lo|, granule of hi, of lo)."""
    E = row_exponent(x)
    xs = np.ldexp(np.asarray(x, np.float32), (HSC - E).astype(np.int32)[..., None])
    assert xs.dtype == np.float32
    hi = _rn_f16(xs)
    lo = None if hi is None else _rn_f16(xs - hi)
    if lo is None:  # values below fp16's normal range: the plain conversions
        hi, lo = [v.astype(np.float32) for v in split_limbs(x, E)]
    hi, lo = np.abs(hi), np.abs(lo)
    return (hi.max(-1).astype(np.float64), lo.max(-1).astype(np.float64), hi.sum(-1, dtype=np.float64),
            lo.sum(-1, dtype=np.float64), _granule32(hi), _granule32(lo))


def _by_granule(stats):
    """Row statistics reduced to one row per distinct (granule of hi, granule of lo): the maxima
    of the other four over the class.  Powers of two: a handful of classes."""
    mh, ml, sh, sl, gh, gl = stats
    _, first, inv = np.unique(np.stack([gh, gl], axis=1), axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    out = []
    for v in (mh, ml, sh, sl):
        m = np.zeros(len(first))
        np.maximum.at(m, inv, v)
        out.append(m)
    return out + [gh[first], gl[first]]


def bound_from_stats(sa, sw):
    """max over (A row, W row) of (max|hi| (sum|hi'| + sum|lo'|) + max|lo| sum|hi'|) / g, taken over
    the rows' granule classes with each class's largest statistics (no smaller, and a
    classes x classes product in place of rows x columns)."""
    amh, aml, _, _, gah, gal = _by_granule(sa)
    _, _, swh, swl, gwh, gwl = _by_granule(sw)
    s = amh[:, None] * (swh + swl)[None, :] + aml[:, None] * swh[None, :]
    return float((s / _pair_granule(gah, gal, gwh, gwl)).max())


def exactness_bound(A, W):
    """An upper bound of  max (sum_k |hi||hi'| + |hi||lo'| + |lo||hi'|) / g  over the outputs of
    one group, g the common granule of an output's terms, from row maxima and row sums alone
    (no matrix product: cheap enough for every case).  Below 2^22 the f16x3 sum is exact in
    fp32 in any order."""
    return bound_from_stats(row_stats(A), row_stats(W))


def exactness_max(A, W):
    """The condition's left side itself (three matrix products), in granules."""
    ah, al = split_limbs(A, row_exponent(A))
    wh, wl = split_limbs(W, row_exponent(W))
    s = np.abs(ah) @ (np.abs(wh) + np.abs(wl)).T + np.abs(al) @ np.abs(wh).T
    return float((s / _pair_granule(granule(ah), granule(al), granule(wh), granule(wl))).max())


# ---- operand builders ---------------------------------------------------------------------------
def _scale_rows(rs, x, common=False):
    """x times a per-row power of two 2^r, r in [-20, 20] (in place: exact in fp32); common: row
    i of every group takes the same r (the groups of an A operand share their leading columns
    under k_shared, so a row's scale cannot depend on the group)."""
    r = rs.randint(-20, 21, size=((1,) if common else x.shape[:1]) + x.shape[1:-1] + (1,))
    x *= np.exp2(r).astype(np.float32)
    return x


def _signs(rs, shape):
    return (rs.randint(0, 2, size=shape, dtype=np.int8) * 2 - 1).astype(np.int8)


def tier1(rs, shape, common=False):
    """Integers |v| <= 15 (at least one nonzero per row) times 2^r, r in [-20, 20] per row."""
    v = rs.randint(-15, 16, size=shape, dtype=np.int8).astype(np.float32)
    dead = ~(v != 0).any(axis=-1)
    v[dead, 0] = 1.0
    return _scale_rows(rs, v, common)


def _two_limb_values(rs, shape):
    p = rs.randint(1, 8, size=shape, dtype=np.int8) * _signs(rs, shape)
    q = _signs(rs, shape)
    q = np.where(np.abs(p) == 1, np.sign(p), q)  # 1024 - 1/4 is a rounding tie in fp16
    out = p.astype(np.float32)
    out *= np.float32(1024.0)
    out += q.astype(np.float32) * np.float32(0.25)
    return out


def _anchor(rs, xs, first=0):
    K = xs.shape[-1]
    col = rs.randint(first, K, size=xs.shape[:-1])
    np.put_along_axis(xs, col[..., None], np.float32(8192.0), axis=-1)


def tier2_a(rs, shape):
    """Dense two-limb rows: 1024 p + q/4 everywhere, one anchor of 8192 per row, times 2^r (r
    common to the groups; the anchor past the first 32 columns when there are more, so a row
    keeps exactly one when its leading columns are another group's)."""
    xs = _two_limb_values(rs, shape)
    _anchor(rs, xs, SHARED if shape[-1] > SHARED else 0)
    return _scale_rows(rs, xs, common=True)


def tier2_w_positions(n, K):
    """The 12 nonzero k of W row n."""
    return (7 * n + np.arange(12) * (K // 12)) % K


def tier2_w(rs, shape):
    """Two-limb rows with 12 nonzeros at (7 n + j (K // 12)) % K and the anchor, times 2^r."""
    G, N, K = shape
    xs = np.zeros(shape, np.float32)
    pos = (7 * np.arange(N)[:, None] + np.arange(12)[None, :] * (K // 12)) % K
    vals = _two_limb_values(rs, (G, N, 12))
    for g in range(G):
        np.put_along_axis(xs[g], pos, vals[g], axis=-1)
    _anchor(rs, xs)
    return _scale_rows(rs, xs)


@functools.lru_cache(maxsize=2)
def _master_a(tier, K):
    """[4][rows][K] A operand of a (tier, K); every case of that pair reads a row prefix."""
    rs = np.random.RandomState(1000 * tier + K)
    shape = (4, MAX_ROWS if K <= 352 else 6144, K)
    a = tier1(rs, shape, common=True) if tier == 1 else tier2_a(rs, shape)
    if K > SHARED:  # the operand as the launch sees it under k_shared: member 0's leading columns
        a[1:, :, :SHARED] = a[0, :, :SHARED]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _a_stats(tier, K):
    return [row_stats(g) for g in _master_a(tier, K)]


@functools.lru_cache(maxsize=None)
def _w_stats(tier, Nw, K):
    return [row_stats(g) for g in _master_w(tier, Nw, K)]


def case_bound(c):
    """exactness_bound of a case, over its groups, from the cached row statistics of its
    operands (the case's zero row only lowers it)."""
    return max(bound_from_stats([v[:c.rows] for v in sa], sw)
               for sa, sw in zip(_a_stats(c.tier, c.K)[:c.groups], _w_stats(c.tier, c.N, c.K)[:c.groups]))


@functools.lru_cache(maxsize=8)
def _master_w(tier, Nw, K):
    rs = np.random.RandomState(7000 * tier + 13 * Nw + K)
    w = tier1(rs, (4, Nw, K)) if tier == 1 else tier2_w(rs, (4, Nw, K))
    w.setflags(write=False)
    return w


# ---- tile selection, restated ---------------------------------------------------------------------
# (BM, BN, threads, LDS bytes) of the tiles whose shape the selection or a workspace needs
TILE = {
    "H256": (256, 256, 512, 163840), "X256": (256, 256, 512, 114688),
    "HS64": (128, 64, 256, 61440), "HS64w8": (128, 64, 512, 61440),
    "HS32": (128, 32, 256, 51200), "HS32w8": (128, 32, 512, 51200),
    "H128x224 stream-K": (128, 224, 896, 112640),
}
SMALL_KT, SMALL_KSMAX = 7, 8


def round_up(x, m):
    return (x + m - 1) // m * m


def resident_wgs(n_cus, lds, nt, occ):
    per_cu = min((160 * 1024) // lds, (occ * 4) // (nt // 64))
    return max(per_cu, 1) * n_cus


def small_plan(groups, rows, N, K, bn):
    """(tiles, workgroups, segments per tile) of the small-row stream-K launch; tiles 0: not covered."""
    if rows <= 0 or rows % 128 or N % bn or K % 32 or groups < 1:
        return 0, 0, 0
    tiles = rows // 128 * (N // bn) * groups
    ks = min(max((K // 32 + SMALL_KT // 2) // SMALL_KT, 1), SMALL_KSMAX)
    return tiles, tiles * ks, ks


def small_hidden(n_cus, groups, rows, N):
    return N % 256 == 0 and rows % 128 == 0 and 2 * (rows // 128) * (N // 256) * groups < n_cus


def small_out(n_cus, S, groups, rows):
    n32 = round_up(S, 32)
    return 128 < n32 <= 224 and rows % 128 == 0 and 2 * (rows // 128) * groups < n_cus


def streamk_tiles(n_cus, S, groups, rows, bm=128):
    """(tiles, workgroups, slots per tile) of the 128 x 224 stream-K output launch; tiles 0: not used."""
    n32 = round_up(S, 32)
    if n32 <= 128 or n32 > 224 or rows % bm:
        return 0, 0, 0
    tiles = rows // bm * groups
    if tiles < n_cus and 2 * tiles >= n_cus:
        return tiles, n_cus, 3
    return 0, 0, 0


def pick_tile(n_cus, epi, groups, rows, N, K, S, split_ws):
    """Name of the tile family a launch takes.  epi: "hidden_h3" / "out_h3" (amx_gemm_bias_act_h3,
    amx_gemm_out_unnorm_h3), "hidden_x6" / "out_x6", "hidden_f32" / "out_f32", "hidden_t64"
    (amx_gemm_bias_act_t64).  N: the hidden layer's columns (ignored by the output entries, which
    derive theirs from S); split_ws: a large enough stream-K workspace is registered.

    A Python copy of the branches in csrc/amx_gemm.hip (and of small_hidden, small_out,
    small_plan, streamk_tiles, resident_wgs): it exists so the case table can say which family
    a shape reaches, and it goes stale if the launchers change without it."""
    n32 = round_up(S, 32)
    if epi == "hidden_t64":
        return "k_gemm64_fwd"
    if epi == "hidden_f32":
        return "T128"
    if epi == "out_f32":
        return "T128x224" if 128 < n32 <= 224 else "T128"
    if epi == "hidden_x6":
        if rows % 256 == 0 and N % 256 == 0 and \
                (rows // 256) * (N // 256) * groups >= resident_wgs(n_cus, TILE["X256"][3], TILE["X256"][2], 2):
            return "X256"
        return "X128"
    if epi == "out_x6":
        return "X128x224" if 128 < n32 <= 224 else "X128"
    if epi == "hidden_h3":
        if rows % 256 == 0 and N % 256 == 0 and K % 32 == 0 and \
                (rows // 256) * (N // 256) * groups >= resident_wgs(n_cus, TILE["H256"][3], TILE["H256"][2], 2):
            return "H256"
        if N % 256 == 0 and K % 32 == 0:
            per = groups * (N // 256)
            if per > 0 and n_cus % per == 0 and rows % (n_cus // per) == 0:
                rb = rows // (n_cus // per)
                if rb in (128, 160, 192, 224):
                    return f"HRow<{rb // 32}>"
        if small_hidden(n_cus, groups, rows, N):
            tiles, _, _ = small_plan(groups, rows, N, K, TILE["HS64"][1])
            if tiles > 0 and split_ws:
                return "HS64w8" if rows == 128 else "HS64"
        return "H128k32" if K % 32 == 0 else "H128"
    assert epi == "out_h3", epi
    nrb = n_cus // (2 * groups) if n_cus % (2 * groups) == 0 else 0
    rb = rows // nrb if nrb > 0 and rows % nrb == 0 else 0
    row_tiles = K % 32 == 0 and rb in (128, 160, 192, 224)
    if 128 < n32 <= 224:
        if K % 32:
            return "H128x224k16"
        if rows % 80 == 0 and groups * (rows // 80) == n_cus:
            return "H80x224"
        if small_out(n_cus, S, groups, rows):
            tiles, _, _ = small_plan(groups, rows, 224, K, TILE["HS32"][1])
            if tiles > 0 and split_ws:
                return "HS32w8" if rows == 128 else "HS32"
        tiles, _, _ = streamk_tiles(n_cus, S, groups, rows)
        if tiles > 0 and split_ws:
            return "H128x224 stream-K"
        if row_tiles:
            return f"HOut<{rb // 32},7>"
        return "H128x224"
    Nn = round_up(S, 128)
    if K % 32 == 0:
        if Nn == 256 and row_tiles:
            return f"HOut<{rb // 32},8>"
        if Nn % 256 == 0:
            return "H128x256"
        return "H128k32"
    return "H128"


def workspace_need(family, groups, rows, N, K):
    """(floats, counters) of the stream-K workspace a family's launch uses; (0, 0): none."""
    if family in ("HS64", "HS64w8", "HS32", "HS32w8"):
        bm, bn = TILE[family][:2]
        tiles, _, ks = small_plan(groups, rows, N, K, bn)
        return tiles * ks * bm * bn, tiles
    if family == "H128x224 stream-K":
        tiles = rows // 128 * groups
        return tiles * 3 * 128 * 224, tiles
    return 0, 0


# ---- the case table -------------------------------------------------------------------------------
Case = namedtuple("Case", "family epi path groups rows N S K k_shared ws tier")
# epi: pick_tile's; path: "h3" / "x6" / "f32"; N: columns computed (hidden: the layer's, output:
# the weight rows, round_up(S, 128)); S: the context's state width; ws: stream-K workspace registered

STREAM_K = ("HS64", "HS64w8", "HS32", "HS32w8", "H128x224 stream-K")


def _shapes():
    """(family, epi, rows, N, S, workspace, K % 32 == 0) of every family at 256 CUs, groups 4."""
    out = [("H256", "hidden_h3", 8192, 512, 197, False, True)]
    out += [(f"HRow<{b}>", "hidden_h3", 1024 * b, 512, 197, False, True) for b in (4, 5, 6, 7)]
    out += [("HS64", "hidden_h3", 256, 512, 197, True, True), ("HS64w8", "hidden_h3", 128, 512, 197, True, True),
            ("H128k32", "hidden_h3", 2048, 512, 197, False, True), ("H128", "hidden_h3", 256, 128, 197, False, False)]
    out += [("H128x224k16", "out_h3", 256, 256, 197, False, False), ("H80x224", "out_h3", 5120, 256, 197, False, True),
            ("HS32", "out_h3", 256, 256, 197, True, True), ("HS32w8", "out_h3", 128, 256, 197, True, True),
            ("H128x224 stream-K", "out_h3", 4096, 256, 197, True, True),
            ("H128x224 stream-K", "out_h3", 6144, 256, 197, True, True)]
    out += [(f"HOut<{b},7>", "out_h3", 1024 * b, 256, 197, False, True) for b in (4, 6, 7)]
    out += [("H128x224", "out_h3", 8192, 256, 197, False, True)]
    out += [(f"HOut<{b},8>", "out_h3", 1024 * b, 256, 226, False, True) for b in (4, 5, 6, 7)]
    out += [("H128x256", "out_h3", 256, 256, 226, False, True)]
    out += [("H128k32", "out_h3", 256, 128, 100, False, True), ("H128k32", "out_h3", 256, 384, 300, False, True),
            ("H128", "out_h3", 256, 128, 100, False, False), ("H128", "out_h3", 256, 384, 300, False, False)]
    return out


def _cases():
    cases = []
    for family, epi, rows, N, S, ws, k32 in _shapes():
        ks = ((32, 0), (96, SHARED), (352, SHARED)) if k32 else ((48, SHARED),)
        if family in STREAM_K:
            ks += ((2304, SHARED),)
        for K, k_shared in ks:
            for tier in (1, 2):
                cases.append(Case(family, epi, "h3", 4, rows, N, S, K, k_shared, ws, tier))
    for family, epi, path, rows, N, S in (
            ("X256", "hidden_x6", "x6", 8192, 512, 197), ("X128", "hidden_x6", "x6", 256, 384, 197),
            ("X128x224", "out_x6", "x6", 256, 256, 197), ("T128", "hidden_f32", "f32", 256, 384, 197),
            ("T128x224", "out_f32", "f32", 256, 256, 197), ("k_gemm64_fwd", "hidden_t64", "f32", 128, 192, 197)):
        for K in (32, 96, 352):
            cases.append(Case(family, epi, path, 4, rows, N, S, K, 0, False, 1))
    # one (tier, K) after the other: the A operand of a pair is built once (_master_a)
    cases.sort(key=lambda c: (c.tier, c.K))
    return cases


CASES = _cases()


def case_id(c):
    fam = c.family.replace("<", "").replace(">", "").replace(",", "_").replace(" ", "_")
    return f"{fam}-{c.epi}-S{c.S}-r{c.rows}-K{c.K}-t{c.tier}"


# ---- one case's inputs and expected outputs ---------------------------------------------------------
COL_OFF, LDC_PAD, LDP_PAD, LD_PAD = 5, 3, 3, 4
SENTINEL = np.float32(-12345.5)


def normalizers(S):
    """(mu_s, sd_s, mu_a, sd_a, mu_d, sd_d) of the test context of state width S: the GEMM
    epilogue reads mu_d and sd_d only.  mu_d is zero on about half the columns (there the
    output is the scaled product alone)."""
    rs = np.random.RandomState(50 + S)
    mu_d = (rs.randn(S) * (rs.rand(S) < 0.5)).astype(np.float32)
    sd_d = rs.uniform(0.5, 2.0, S).astype(np.float32)
    one, zero = np.ones(S, np.float32), np.zeros(S, np.float32)
    return zero, one, np.zeros(A_DIM, np.float32), np.ones(A_DIM, np.float32), mu_d, sd_d


def case_inputs(c):
    """Host arrays of a case.

    A_dev  [G][rows][K + 4]: what the launch reads; the pad columns and, with k_shared,
           members 1..'s first k_shared columns hold NaN (member 0's are the ones used)
    A      [G][rows][K] effective operand (member 0's shared columns in every member)
    W_dev  [G][N][K + 4] (NaN pad), W [G][N][K];  bias [G][N]
    One A row (rows - 3) is all zero."""
    G, rows, N, K = c.groups, c.rows, c.N, c.K
    A = np.array(_master_a(c.tier, K)[:G, :rows])
    W = np.asarray(_master_w(c.tier, N, K)[:G])
    zr = rows - 3
    A[:, zr] = 0.0
    assert c.k_shared in (0, SHARED) and c.k_shared < K
    A_dev = np.full((G, rows, K + LD_PAD), np.nan, np.float32)
    A_dev[:, :, :K] = A
    if c.k_shared:
        A_dev[1:, :, :c.k_shared] = np.nan
    W_dev = np.full((G, N, K + LD_PAD), np.nan, np.float32)
    W_dev[:, :, :K] = W
    # a bias on about half the columns, of the size of a typical product of rows scaled by 2^0;
    # the other columns show the accumulator alone
    rs = np.random.RandomState(c.rows + 3 * c.K + c.tier)
    wscale = np.exp2(row_exponent(W).astype(np.float64))
    ascale = 2.0 ** 4 if c.tier == 1 else 2.0 ** 14
    bias = (rs.randn(G, N) * (rs.rand(G, N) < 0.5) * wscale * ascale).astype(np.float32)
    return dict(A=A, A_dev=A_dev, W=W, W_dev=W_dev, bias=bias, zero_row=zr)


def expected(c, inp):
    """(values [G][rows][N or S], row-exponent output [G][rows] or None) of a case."""
    vals, exps = [], []
    mu_d, sd_d = normalizers(c.S)[4:]
    for g in range(c.groups):
        pre = pre_bias(inp["A"][g], inp["W"][g], c.path)
        if c.epi.startswith("hidden"):
            v, e = hidden_epilogue(pre, inp["bias"][g])
            exps.append(e)
        else:
            v = output_epilogue(pre[:, :c.S], inp["bias"][g, :c.S], sd_d, mu_d)
        vals.append(v)
    return np.stack(vals), (np.stack(exps) if exps else None)
