"""Plain numpy restatement, per trajectory, of what csrc/amx_gae.hip computes (the comparator of
test_cpu_gae_ref.py and test_gpu_gae_edges.py): mjrl's MLPBaseline._features, compute_returns,
compute_advantages and the whitening of BatchREINFORCE.process_paths.  Paths are relative to
mjrl/mjrl/.  No torch, no device, and nothing from oracle.milo_ref (the CPU test pins the two
to each other).

Written from the behaviour of the cited lines with numpy's own dtypes, so that promotion does
the work it does in the reference.  One thing is stated instead of inherited: the reference's
pinned numpy 1.21 promotes `float32 scalar + python float` to float64 inside discount_sum
(utils/process_samples.py:41); numpy 2 would keep float32, so `discount_sum` widens its input
first (as tests/golden/make_golden.py does for G9).

`split` is the one place that knows the segment grid (include/amx_hip.h); everything else
takes one trajectory.
"""
import math
from fractions import Fraction

import numpy as np

LD_WIDER = np.finfo(np.longdouble).nmant > 52


def split(T, L, len_, base, stride, end, t0):
    """The trajectories of a segment grid, in lane order then time order, as
    (row indices, terminated, start position).  Lane l owns rows base[l] + t * stride for
    t < len[l] (base None -> l, len None -> T).  A trajectory ends at a nonzero end flag or at
    the lane's last row; it is terminated only where that flag is 1 (0 at the last row and 2
    anywhere mean cut: bootstrapped from its own last value).  t0[l] is the position of the
    lane's first row; every later trajectory of the lane starts at 0."""
    out = []
    for l in range(L):
        n = T if len_ is None else int(len_[l])
        rows = np.array([(l if base is None else int(base[l])) + t * stride for t in range(n)], dtype=np.int64)
        start, pos = 0, 0 if t0 is None else int(t0[l])
        for t in range(n):
            if end[rows[t]] != 0 or t == n - 1:
                out.append((rows[start:t + 1], bool(end[rows[t]] == 1), pos))
                start, pos = t + 1, 0
    return out


def features(obs, S, kf, positions):
    """MLPBaseline._features (baselines/mlp_baseline.py:36-58) of one trajectory's rows followed
    by predict's / fit's astype('float32') (:65, :100): obs [n, >= S] float64, positions [n] the
    rows' positions in the trajectory (np.arange(l), :54, plus the start).  -> [n, kf] float32,
    columns S+4 .. kf-1 zero (the GEMM's K padding, not part of the reference)."""
    obs = np.asarray(obs, dtype=np.float64)[:, :S]
    with np.errstate(all="ignore"):
        o = np.clip(obs, -10, 10) / 10.0                      # :41
        feat = np.ones((obs.shape[0], S + 4))                 # :46
        feat[:, :S] = o                                       # :49
        al = np.asarray(positions) / 1000.0                   # :54
        for j in range(4):
            feat[:, -4 + j] = al ** (j + 1)                   # :56
        out = np.zeros((obs.shape[0], kf), dtype=np.float32)
        out[:, :S + 4] = feat.astype("float32")
    return out


def discount_sum(x, gamma):
    """utils/process_samples.py:37-44 under numpy 1.21 promotion: float64 running sum."""
    x = np.asarray(x, dtype=np.float64)
    y, run_sum = [], 0.0
    with np.errstate(all="ignore"):
        for t in range(len(x) - 1, -1, -1):
            run_sum = x[t] + gamma * run_sum                  # :41
            y.append(run_sum)
    return np.array(y[::-1], dtype=np.float64)


def returns(rew_f32, gamma):
    """compute_returns (utils/process_samples.py:3-5) of one trajectory -> float64."""
    assert rew_f32.dtype == np.float32
    return discount_sum(rew_f32, float(gamma))


def standard_mode(lam):
    """compute_advantages' switch (utils/process_samples.py:10)."""
    return lam is None or lam < 0.0 or lam > 1.0


def deltas(rew_f32, v_f32, terminated, gamma):
    """td_deltas (utils/process_samples.py:25, 28) with numpy's promotion: np.append(b, 0.0) is
    float64 (so are the deltas of a terminated trajectory), np.append(b, b[-1]) stays float32
    (the python float gamma is cast to float32 and every op rounds to float32)."""
    assert rew_f32.dtype == np.float32 and v_f32.dtype == np.float32
    b1 = np.append(v_f32, 0.0 if terminated else v_f32[-1])
    with np.errstate(all="ignore"):
        return rew_f32 + float(gamma) * b1[1:] - b1[:-1]


def advantages(rew_f32, v_f32, terminated, gamma, lam):
    """compute_advantages (utils/process_samples.py:7-29, normalize off) of one trajectory ->
    float64: returns - baseline in the standard mode, else the discounted sum of the deltas."""
    if standard_mode(lam):
        with np.errstate(all="ignore"):
            return returns(rew_f32, gamma) - v_f32            # :13
    return discount_sum(deltas(rew_f32, v_f32, terminated, gamma), float(gamma) * float(lam))  # :29


def _round_f32(fr):
    """A Fraction rounded once to float32 (float(fr) is correctly rounded to float64; where that
    second rounding lands on the wrong side, a neighbour is nearer)."""
    f = np.float32(float(fr))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min((c for c in cands if np.isfinite(c)), key=lambda c: abs(Fraction(float(c)) - fr))


def deltas_mutant(rew_f32, v_f32, terminated, gamma, kind):
    """What the deltas would be under a substitution the tests must be able to see (finite
    inputs): kind 'swap' computes a terminated trajectory's deltas in float32 and a cut one's in
    float64; kind 'fma' fuses the multiply and the add (x + gamma * b_next rounded once)."""
    n = len(rew_f32)
    nxt = np.append(v_f32[1:], np.float32(0.0) if terminated else v_f32[-1]).astype(np.float32)
    f32 = (not terminated) != (kind == "swap")
    out = np.empty(n, dtype=np.float64)
    for t in range(n):
        x, b, bn = rew_f32[t], v_f32[t], nxt[t]
        if f32:
            g = np.float32(gamma)
            s = _round_f32(Fraction(float(x)) + Fraction(float(g)) * Fraction(float(bn))) if kind == "fma" \
                else np.float32(x + np.float32(g * bn))
            out[t] = np.float32(s - b)
        else:
            s = float(Fraction(float(x)) + Fraction(float(gamma)) * Fraction(float(bn))) if kind == "fma" \
                else float(x) + float(gamma) * float(bn)
            out[t] = s - float(b)
    return out


def head(h_f32, w_f32, b_f32):
    """The model's last Linear(H -> 1) (baselines/mlp_baseline.py:20-27) of one row as the exact
    dot product: float32 x float32 products are exact in float64, math.fsum adds them without
    error, the sum is rounded to float32 and b added in float32.  -> (v float32, s the float64
    dot, mag = sum |h_k w_k|)."""
    assert h_f32.dtype == np.float32 and w_f32.dtype == np.float32
    p = h_f32.astype(np.float64) * w_f32.astype(np.float64)
    s = math.fsum(p)
    with np.errstate(all="ignore"):
        v = np.float32(np.float32(s) + np.float32(b_f32))
    return v, s, math.fsum(np.abs(p))


def whiten(x, eps):
    """(x - mean) / (std + eps), population std (algos/batch_reinforce.py:284-285;
    utils/process_samples.py:15-19 with eps 1e-8), in more than float64: np.longdouble where it is
    wider (64-bit significand, pairwise sums), else exact rational sums.  -> (out, mean, std)
    rounded to float64 at the end; an empty input gives mean = std = 0."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size == 0:
        return x.copy(), 0.0, 0.0
    if LD_WIDER:
        xl = x.astype(np.longdouble)
        mean = np.sum(xl) / np.longdouble(x.size)
        d = xl - mean
        sd = np.sqrt(np.sum(d * d) / np.longdouble(x.size))
        return (d / (sd + np.longdouble(eps))).astype(np.float64), float(mean), float(sd)
    xs = [Fraction(float(v)) for v in x]
    mean = sum(xs) / x.size
    d = np.array([float(v - mean) for v in xs])
    sd = math.sqrt(math.fsum(d * d) / x.size)
    return d / (sd + eps), float(mean), sd
