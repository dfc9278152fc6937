"""Plain CPU reference of the reward kernels in csrc/amx_cost.hip (numpy/torch, no device code).

Two kinds of operands:

* exact_case / exact_head: every entry is k/64 with a small integer k, so every product is a
  multiple of 2^-12 and every dot product and sum is the same real number in any summation
  order.  A kernel that drops, repeats or misplaces a term cannot hide behind rounding: all
  outputs are compared bit for bit.
* real_case / real_head: the cos(u)*sqrt(2/F) rows of tests/test_gpu_relabel_fused.py.  There
  the fp64 dot depends on the order, so `dot32` also returns the rows (`near`) where the
  longdouble dot +- F*2^-53*sum|p_i w_i| (the standard fp64 dot-product bound, any order)
  rounds to two different fp32 values; only those rows may take the other candidate.

The scalar algebra after the dot is done in separate fp32 numpy ops in the order of
linear_cost.py:102-147, batch_reinforce.py:144 and gail_cost.py:231-279.
"""
import numpy as np
import torch

LD = np.longdouble
f32 = np.float32
U64 = 2.0 ** -53

# ---- the shapes both test files use ---------------------------------------------------------
REWARD_F = [128, 256, 384, 512, 768, 1024, 1152, 4096]
REWARD_N = [1, 7, 31, 32, 33, 257]
REWARD_ROWS = max(REWARD_N)
# rows per wave of k_mmd_relabel<NC> at each width
RELABEL_R = {256: 8, 512: 4, 768: 2, 1024: 2}
EXPERT_SMALL = [(F, n_e) for F in (128, 512) for n_e in (1, 3, 16, 17, 63, 16384, 16385)]
EXPERT_PIPE = [(F, m * 4096 * R + d) for F, R in ((256, 8), (768, 2), (1024, 2), (384, 1))
               for m, d in ((1, 0), (1, 1), (2, 4097))]
EXPERT_CASES = EXPERT_SMALL + EXPERT_PIPE
PARTS_N = [0, 1, 63, 64, 65, 1280]
PARTS_F = [16, 128, 520]
FIT_F = [128, 384, 4096]
HEAD_HD = [1, 63, 64, 65, 512]
HEAD_N = [1, 5, 260]
HEAD_ROWS = max(HEAD_N)
HEAD_LOGITS = [0.0, 1e-4, -1e-4, 20.0, -20.0, 100.0, -100.0]  # the first rows' logits when b3 = 0
LAM, THR, C_MIN, C_MAX = 0.0025, 0.07, -1.0, 0.0


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(a, b):
    """Bit equality of two float arrays; NaNs only have to sit at the same positions."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# ---- operands --------------------------------------------------------------------------------
def _target_rows(rs, n, d, lo=-2.0, hi=1.0, amp=3.0):
    """n rows of integers k (|k| <= 63) with sum_f k*d/4096 spread over about [lo, hi]: the row's
    target t is uniform, k = rint(t*4096/sum(d^2)*d + dither)."""
    t = rs.uniform(lo, hi, (n, 1))
    g = 4096.0 / float(np.sum(d.astype(np.float64) ** 2))
    k = np.rint(t * g * d[None, :] + rs.uniform(-amp, amp, (n, d.shape[0])))
    return np.clip(k, -63, 63)


def exact_case(F, n, n_e, seed):
    """Exactly summable relabel operands.  count = 1024, msg[f] = 16*i, phi_e[f] = j/64, so
    w = (i - j)/64 with |i - j| <= 8; rows are k/64.  Row dots are multiples of 2^-12 of size
    < 4 (exact in fp32), spread over about [-2, 1] so both clamp bounds cut a third of the rows;
    the clamped expert terms are multiples of 2^-12 in [-1, 0] and their fp64 sum is exact."""
    rs = np.random.RandomState(1000 + seed)
    d = rs.randint(-8, 9, F)
    d[d == 0] = 1
    j = rs.randint(-30, 31, F)
    i = j + d
    out = {
        "F": F, "count": 1024.0,
        "msg": np.concatenate([16.0 * i, [1024.0]]).astype(np.float64),
        "phi_e": (j / 64.0).astype(f32),
        "phi": (_target_rows(rs, n, d) / 64.0).astype(f32),
        "erows": (_target_rows(rs, n_e, d) / 64.0).astype(f32),
        "disc": (rs.uniform(0.0, 0.2, n)).astype(f32),
    }
    return out


def real_case(F, n, n_e, seed):
    """The inputs of tests/test_gpu_relabel_fused.py: cos(u)*sqrt(2/F) rows, phi_e the fp32 of the
    expert rows' fp64 mean, msg the fp64 column sum of the rollout rows (count = n)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sc = float(np.sqrt(2.0 / F))
    phi = torch.cos(torch.rand(n, F, generator=g) * 6.3) * sc
    erows = torch.cos(torch.rand(n_e, F, generator=g) * 6.3 + 0.3) * sc
    phi_e = erows.double().mean(0).float()
    disc = torch.rand(n, generator=g) * 0.2
    msg = torch.cat([phi.double().sum(0), torch.tensor([float(n)], dtype=torch.float64)])
    return {"F": F, "count": float(n), "msg": msg.numpy(), "phi_e": phi_e.numpy(), "phi": phi.numpy(),
            "erows": erows.numpy(), "disc": disc.numpy()}


def make_case(kind, F, n, n_e, seed):
    return (exact_case if kind == "exact" else real_case)(F, n, n_e, seed)


def reward_case(kind, F):
    """The reward-row case of a width: REWARD_ROWS rows (the tests score the first n)."""
    return make_case(kind, F, REWARD_ROWS, 64, 0)


def expert_case(kind, F, n_e):
    """The expert-cost case of a width and row count (7 rollout rows ride along)."""
    return make_case(kind, F, 7, n_e, 1)


def witness(case):
    """The case's w (mmd_fit of its message)."""
    return mmd_fit(case["msg"], 0.0, case["phi_e"])[0]


# ---- the dot and its candidates ----------------------------------------------------------------
def dot32(rows, w, chunk=4096):
    """fp32 rounding of the longdouble row dots.  Returns (d, lo, hi, near): d the rounded dot,
    lo/hi the roundings of dot -+ K*2^-53*sum|p_i w_i|, near = lo != hi (rows whose fp32 dot an
    fp64 summation in another order may round to the neighbour)."""
    rows = np.asarray(rows, f32)
    w = np.asarray(w, f32)
    K = rows.shape[1]
    wl = w.astype(LD)
    d = np.empty(rows.shape[0], LD)
    a = np.empty(rows.shape[0], LD)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, rows.shape[0], chunk):
            p = rows[s:s + chunk].astype(LD) * wl[None, :]
            d[s:s + chunk] = p.sum(1)
            a[s:s + chunk] = np.abs(p).sum(1)
        bnd = a * LD(K * U64)
        d32, lo, hi = d.astype(f32), (d - bnd).astype(f32), (d + bnd).astype(f32)
    fin = np.isfinite(a.astype(np.float64))
    lo, hi = np.where(fin, lo, d32), np.where(fin, hi, d32)
    return d32, lo, hi, bits(lo) != bits(hi)


def row_dots_f64(rows, w, order):
    """fp64 row dots summed one term at a time in a given order: 'forward', 'reversed', or
    'lanes' (lane l of 64 takes floats 4l .. 4l+3 of every 256, then the lanes are added)."""
    p = np.asarray(rows, np.float64) * np.asarray(w, np.float64)[None, :]
    K = p.shape[1]
    if order == "lanes":
        acc = np.zeros((p.shape[0], 64))
        for c in range(0, K, 256):
            for e in range(4):
                cols = c + 4 * np.arange(64) + e
                ok = cols < K
                acc[:, ok] = acc[:, ok] + p[:, cols[ok]]
        p, K = acc, 64
    s = np.zeros(p.shape[0])
    for f in (range(K - 1, -1, -1) if order == "reversed" else range(K)):
        s = s + p[:, f]
    return s


# ---- scalar algebra ------------------------------------------------------------------------
def clamp32(v, lo, hi):
    """torch.clamp(min, max): the min bound first, then the max; NaN propagates."""
    v = np.asarray(v, f32)
    v = np.where(v < f32(lo), f32(lo), v)
    return np.where(v > f32(hi), f32(hi), v).astype(f32)


def reward_algebra(d32, disc, thr, lam, c_min, c_max, clamp):
    """linear_cost.py:102-147 and batch_reinforce.py:144 on a given fp32 dot."""
    d32, disc = np.asarray(d32, f32), np.asarray(disc, f32)
    one_m = f32(1.0 - float(lam))          # (1 - lambda) formed in double, then rounded
    lam32 = f32(lam)
    with np.errstate(invalid="ignore", over="ignore"):
        if clamp:
            v = clamp32(d32, c_min, c_max)                           # :102
            dh = (disc / f32(thr)).astype(f32)                       # :132
            dh = np.where(dh > f32(1.0), f32(1.0), dh).astype(f32)   # :134
            bonus = (dh * f32(c_min)).astype(f32)                    # :136
        else:
            v, bonus = d32, disc                                     # :103, :139
        ipm = (one_m * v).astype(f32)                                # :141
        wb = (lam32 * bonus).astype(f32)                             # :144
        cost = (ipm - wb).astype(f32)                                # :147
        reward = (f32(-1.0) * cost).astype(f32)                      # batch_reinforce.py:144
    return reward, ipm, wb


def rewards(phi, w, disc, thr, lam, c_min, c_max, clamp):
    """reward, ipm, wb, near of the rows; `near` as in dot32."""
    d, _, _, near = dot32(phi, w)
    return (*reward_algebra(d, disc, thr, lam, c_min, c_max, clamp), near)


def reward_candidates(phi, w, disc, thr, lam, c_min, c_max, clamp):
    """The (reward, ipm, wb) triples of the two candidate dots, and near."""
    _, lo, hi, near = dot32(phi, w)
    return (reward_algebra(lo, disc, thr, lam, c_min, c_max, clamp),
            reward_algebra(hi, disc, thr, lam, c_min, c_max, clamp), near)


def mmd_fit(msg, count, phi_e):
    """w = float32(msg/count) - phi_e, float32(sum w^2) with its two candidates and near."""
    msg = np.asarray(msg, np.float64)
    F = np.asarray(phi_e).shape[0]
    c = float(count) if count else float(msg[F])
    w = ((msg[:F] / c).astype(f32) - np.asarray(phi_e, f32)).astype(f32)
    m, lo, hi, near = dot32(w[None, :], w)
    return w, m[0], lo[0], hi[0], bool(near[0])


def expert_cost(erows, w, lam, c_min, c_max):
    """sum_r clamp(float32(row.w)) and (1 - lambda)*float32(sum/n).  Also the clamped terms, the
    near mask and the bound n*2^-53*sum|c_r| + sum_near ulp32(c_r) on an fp64 sum in any order."""
    d, _, _, near = dot32(erows, w)
    c = clamp32(d, c_min, c_max)
    n = c.shape[0]
    tot = float(c.astype(LD).sum())
    mean = expert_mean(tot, n, lam)
    bound = n * U64 * float(np.abs(c).astype(LD).sum()) + float(np.spacing(np.abs(c[near])).astype(LD).sum())
    return tot, mean, c, near, bound


def expert_mean(tot, n, lam):
    return f32(f32(1.0 - float(lam)) * f32(np.float64(tot) / np.float64(n)))


def expert_blocks(n):
    return min(1024, max(1, (n + 15) // 16))


def expert_partials(c):
    """Block partials of the expert sum: block b takes rows (r // 4) % ne == b."""
    ne = expert_blocks(c.shape[0])
    out = np.zeros(ne, np.float64)
    np.add.at(out, (np.arange(c.shape[0]) // 4) % ne, c.astype(np.float64))
    return out


# ---- discriminator head ------------------------------------------------------------------------
def _special_rows(h):
    for r, t in enumerate(HEAD_LOGITS[:h.shape[0]]):
        h[r] = 0.0
        h[r, 0] = t
    return h


def exact_head(Hd, n, seed):
    """h rows k/64, w3 = j/64 with w3[0] = 1: the head dot is a multiple of 2^-12 of size < 2^11,
    exact in fp32 in any order.  The first rows are [t, 0, ...] with t from HEAD_LOGITS."""
    rs = np.random.RandomState(2000 + seed)
    a = int(min(63, np.sqrt(18432.0 / np.sqrt(Hd))))
    h = (rs.randint(-a, a + 1, (n, Hd)) / 64.0).astype(f32)
    w3 = (rs.randint(-a, a + 1, Hd) / 64.0).astype(f32)
    w3[0] = 1.0
    return {"h": _special_rows(h), "w3": w3, "disc": rs.uniform(0.0, 0.2, n).astype(f32)}


def real_head(Hd, n, seed):
    rs = np.random.RandomState(3000 + seed)
    h = np.maximum(rs.randn(n, Hd), 0.0).astype(f32)
    w3 = (rs.uniform(-1.0, 1.0, Hd) * 2.0 / np.sqrt(Hd)).astype(f32)
    w3[0] = 1.0
    return {"h": _special_rows(h), "w3": w3, "disc": rs.uniform(0.0, 0.2, n).astype(f32)}


def make_head(kind, Hd, n, seed):
    return (exact_head if kind == "exact" else real_head)(Hd, n, seed)


def ll_reward_f32(D):
    """-logsigmoid(D) = -(min(D, 0) - log1p(exp(-|D|))), each op a separate torch-CPU fp32 op."""
    D = torch.from_numpy(np.ascontiguousarray(D, f32))
    r = -(torch.clamp(D, max=0.0) - torch.log1p(torch.exp(-torch.abs(D))))
    return r.numpy()


def ll_reward_ld(D):
    """The same formula in longdouble on the fp32 logits."""
    D = np.asarray(D, f32).astype(LD)
    return -(np.minimum(D, LD(0)) - np.log1p(np.exp(-np.abs(D))))


def disc_algebra(D, loss, disc, lam, rew=None):
    """gail_cost.py:231-279 on given fp32 logits: returns (reward, rew) where rew = -cost of the
    loss (`rew` given: the loss term is taken from it) and reward follows the disc / None path."""
    D = np.asarray(D, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        if rew is None:
            if loss == 0:
                om = (f32(1.0) - D).astype(f32)            # :234
                q = (f32(0.25) * (om * om).astype(f32)).astype(f32)
                rew = (f32(1.0) - q).astype(f32)
                rew = np.where(rew < f32(0.0), f32(0.0), rew).astype(f32)   # :235
            else:
                rew = ll_reward_f32(D)
        if disc is None:
            return rew, rew
        ipm = (f32(1.0 - float(lam)) * (-rew).astype(f32)).astype(f32)      # :269
        bonus = (f32(lam) * np.asarray(disc, f32)).astype(f32)             # :273
        return (f32(-1.0) * (ipm - bonus).astype(f32)).astype(f32), rew


def disc_reward(h, w3, b3, loss, disc, lam):
    """reward, logits, near of the head rows (logits = float32(h.w3) + b3)."""
    d, _, _, near = dot32(h, w3)
    D = (d + f32(b3)).astype(f32)
    return disc_algebra(D, loss, disc, lam)[0], D, near


def logit_candidates(h, w3, b3):
    d, lo, hi, near = dot32(h, w3)
    return (lo + f32(b3)).astype(f32), (hi + f32(b3)).astype(f32), near


# ---- column sums and cost rows -------------------------------------------------------------------
def colsum(parts, F):
    """Column sums of fp64 partial rows (longdouble, rounded to fp64)."""
    parts = np.asarray(parts, np.float64).reshape(-1, F)
    return parts.astype(LD).sum(0).astype(np.float64) if parts.shape[0] else np.zeros(F)


def int_parts(n_parts, F, seed):
    """Integer-valued fp64 partial rows: any summation order is exact."""
    rs = np.random.RandomState(4000 + seed)
    return rs.randint(-2 ** 20, 2 ** 20, (n_parts, F)).astype(np.float64)


def cost_rows(segs, widths, ldc):
    """float32 [x0[:, :w0], x1[:, :w1], x2[:, :w2], 0 ...] up to ldc."""
    B = max([s.shape[0] for s, w in zip(segs, widths) if w] + [0])
    out = np.zeros((B, ldc), f32)
    o = 0
    for s, w in zip(segs, widths):
        if w:
            out[:, o:o + w] = np.asarray(s, np.float64)[:, :w].astype(f32)
        o += w
    return out
