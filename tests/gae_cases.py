"""Inputs shared by test_cpu_gae_ref.py (which measures numpy on them) and test_gpu_gae_edges.py
(which runs the device on them): the whitening inputs with the allowance derived from numpy's own
error, and the returns / GAE grids with their rewards and values.  Plain numpy, seeded."""
import numpy as np

U = 2.0 ** -53
EPS = 1e-6

# ---- whitening ---------------------------------------------------------------------------------
# Largest error of numpy's own float64 (x - x.mean()) / (x.std() + eps) against gae_ref.whiten
# over `whiten_cases()`, as measured by test_cpu_gae_ref.py::test_whitening_yardstick (which
# asserts the measurement does not exceed these, so the allowance cannot drift from it):
#   per element, in units of 2^-53 (|x| + |mean|) / (sd + eps);  mean in 2^-53 |mean|;  sd in 2^-53 sd.
NUMPY_MAX = {"elem": 3.1, "mean": 1.7, "sd": 3.9}  # measured 3.04 (flat1023), 1.66 (emptychunk), 3.86 (ill1e6)
# The device sums in another fixed order (thread strides, wave butterflies, 16 wave parts, chunks
# in order) than numpy's pairwise blocks of 128: a different rounding-error sample of the same
# depth, taken as up to 4x numpy's.  Where |mean| >> sd the std's error is quadratic in the mean's
# (the squared deviations about a mean off by dm sum to n dm^2 too much: d sd / sd = (dm / sd)^2 / 2),
# so 4x on the mean is 16x there.  Set before any device run; the device then measured 3.68 / 1.54 / 3.86.
MARGIN = {"elem": 4.0, "mean": 4.0, "sd": 16.0}
ALLOW = {k: NUMPY_MAX[k] * MARGIN[k] for k in NUMPY_MAX}


def grid_rows(T, L, len_, base, stride):
    """Row index of every valid cell (t, l), and the cell's flat index i = t * L + l."""
    rows, cells = [], []
    for l in range(L):
        n = T if len_ is None else int(len_[l])
        for t in range(n):
            rows.append((l if base is None else int(base[l])) + t * stride)
            cells.append(t * L + l)
    return np.array(rows, dtype=np.int64), np.array(cells, dtype=np.int64)


def _wcase(name, T, L, x_of, len_=None, base=None, stride=None, size=None, seed=0):
    stride = L if stride is None else stride
    rows, cells = grid_rows(T, L, len_, base, stride)
    size = int(rows.max(initial=-1)) + 1 if size is None else size
    buf = np.full(max(size, 1), np.nan)
    buf[rows] = x_of(np.random.RandomState(seed), len(rows))
    return dict(name=name, T=T, L=L, len=None if len_ is None else np.asarray(len_, np.int32),
                base=None if base is None else np.asarray(base, np.int64), stride=stride, buf=buf, rows=rows,
                cells=cells)


def _randn(rs, n):
    return rs.randn(n) * 3.0 + 0.7


def whiten_cases():
    """Every whitening input of the GPU test: dicts with the grid (T, L, len, base, stride), `buf`
    (the float64 row space; cells outside the grid hold NaN), `rows` (the grid's rows) and `cells`."""
    out = []
    for n in (1, 2, 1023, 1024, 1025, 4096, 8193):
        out.append(_wcase(f"flat{n}", 1, n, _randn, seed=n))
    rl = np.random.RandomState(5).randint(0, 1301, size=7)
    rl[[0, 1, 2, 5]] = [0, 1, 1300, 1300]
    out.append(_wcase("ragged1300x7", 1300, 7, _randn, len_=rl, size=1300 * 7, seed=11))
    # concatenated-paths layout whose cells t >= 1500 are all invalid: chunks 1..3 of 4096 are empty
    out.append(_wcase("emptychunk", 7000, 2, _randn, len_=[1500, 300], base=[0, 1500], stride=1, size=1800, seed=12))
    # one row of 8200 lanes whose first 4096 are empty: chunk 0 has no valid cell (its mean is no shift for the
    # others'), on ill-conditioned values
    out.append(_wcase("leadempty", 1, 8200, lambda rs, n: 1e6 + 1e-3 * rs.randn(n), len_=[0] * 4096 + [1] * 4104,
                      size=8200, seed=13))
    for T in (3, 9):
        for pad in (0, 31):
            out.append(_wcase(f"engine{T}x257+{pad}", T, 257, _randn, stride=257 + pad, size=T * (257 + pad),
                              seed=20 + T + pad))
    out.append(_wcase("T0", 0, 5, _randn, size=8))
    out.append(_wcase("L0", 5, 0, _randn, stride=1, size=8))
    out.append(_wcase("len0", 4, 3, _randn, len_=[0, 0, 0], size=12))
    out.append(_wcase("const", 1, 5000, lambda rs, n: np.full(n, 0.75)))
    out.append(_wcase("ill1e6", 1, 9001, lambda rs, n: 1e6 + 1e-3 * rs.randn(n), seed=31))
    out.append(_wcase("ill-3e8", 1, 9001, lambda rs, n: -3e8 + rs.randn(n), seed=32))
    return out


def whiten_errors(x, out, mean, sd, ref_out, ref_mean, ref_sd, eps):
    """(elem, mean, sd) errors in the units above; an error against a zero unit is 0 if exact, inf if not."""
    def units(err, unit):
        err, unit = np.asarray(err, np.float64), np.asarray(unit, np.float64)
        with np.errstate(all="ignore"):
            r = np.where(err == 0.0, 0.0, np.where(unit > 0.0, err / unit, np.inf))
        return float(np.max(r, initial=0.0))
    with np.errstate(all="ignore"):
        e = units(np.abs(out - ref_out), U * (np.abs(x) + abs(ref_mean)) / (ref_sd + eps))
    return e, units(abs(mean - ref_mean), U * abs(ref_mean)), units(abs(sd - ref_sd), U * ref_sd)


# ---- returns / GAE -----------------------------------------------------------------------------
GAMMA_LAMBDA = [(0.995, 0.97), (1.0, 1.0), (0.0, 0.97), (0.9, 0.0), (0.995, None), (0.995, 1.5), (0.995, -0.1)]
END_PATTERNS = ["none", "every", "last", "random", "two"]


def end_flags(pattern, T, L, len_, base, stride, nrows, seed=0):
    """uint8 end flags over the row space for one of END_PATTERNS."""
    rs = np.random.RandomState(seed)
    end = np.zeros(nrows, dtype=np.uint8)
    for l in range(L):
        n = T if len_ is None else int(len_[l])
        r = np.array([(l if base is None else int(base[l])) + t * stride for t in range(n)], dtype=np.int64)
        if n == 0:
            continue
        if pattern == "every":
            end[r] = 1
        elif pattern == "last":
            end[r[-1]] = 1
        elif pattern == "random":
            end[r] = rs.rand(n) < 0.3
        elif pattern == "two":  # 2 in the middle of a lane (and at some last rows), 1 elsewhere at p = 0.2
            end[r] = np.where(rs.rand(n) < 0.2, 1, 0)
            end[r[rs.randint(0, n)]] = 2
            if n > 2:
                end[r[n // 2]] = 2
    return end


def gae_values(nrows, seed):
    """float32 rewards and values per row: randn-sized, so gamma * b + r rounds in float32 (the
    float32 and float64 delta paths differ, and so would a fused multiply-add)."""
    rs = np.random.RandomState(seed)
    return (rs.randn(nrows) * 0.3).astype(np.float32), rs.randn(nrows).astype(np.float32)
