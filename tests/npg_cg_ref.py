"""Plain reference of the NPG solve half of csrc/amx_npg.hip: the conjugate-gradient start and step
(mjrl/mjrl/utils/cg_solve.py:3-23 under the kernels' contract), the column sums of the pass's
partials, the log_std curvature (gaussian_mlp.py:144-155 with Dr's 1e-8) and the step after the
solve (npg_cg.py:141-163, gaussian_mlp.py:71-94).  numpy and Python only: nothing here knows of
blocks, runs, waves or any summation order.

Every sum (p.z, r'.r', b.b, vpg.npg, a column of partials) is the exact real sum of the exact
products, rounded once: each product is split into its rounded value and its exact remainder
(Dekker's two-product; checked against fractions.Fraction in tests/test_cpu_npg_cg_ref.py) and
math.fsum adds the 2n pieces without error.  Beside every sum comes sum|terms|, the magnitude the
tests' bounds are stated in.  Everything elementwise is one IEEE float64 operation per arithmetic
sign of the contract, never fused.
"""
import math
from fractions import Fraction

import numpy as np

_SPLIT = 134217729.0  # 2^27 + 1


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (no overflow, no underflow of e)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dot(a, b):
    """(sum a_i b_i rounded once, sum |a_i b_i|)."""
    p, e = two_prod(a, b)
    return math.fsum(np.concatenate([p.ravel(), e.ravel()]).tolist()), math.fsum(np.abs(p).ravel().tolist())


def dot_fraction(a, b):
    """dot()'s first value from rational arithmetic (slow: the check of two_prod)."""
    return float(sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0)))


def div(a, b):
    return float(np.float64(a) / np.float64(b))  # IEEE: inf / nan instead of ZeroDivisionError


def fma(a, b, c):
    """fl(a b + c), one rounding."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def axpy_candidates(c, a, b, got, dtype=np.float64):
    """The two IEEE readings of c + a * b per element (a scalar): fl(c + fl(a b)) and the fused
    fl(c + a b), in float64.  Returns (unfused, fused), the fused one evaluated (rationally) only
    where `got` differs from the unfused one rounded to `dtype` (the format `got` was stored in) --
    elsewhere it is set to the unfused value, which `got` equals."""
    c, b, got = (np.asarray(v, np.float64) for v in (c, b, got))
    with np.errstate(invalid="ignore", over="ignore"):
        unf = c + np.float64(a) * b
        seen = unf.astype(dtype).astype(np.float64)
    fus = unf.copy()
    for i in np.nonzero(~((got == seen) | (np.isnan(got) & np.isnan(seen))))[0]:
        if math.isfinite(c[i]) and math.isfinite(b[i]) and math.isfinite(a):
            fus[i] = fma(a, b[i], c[i])
    return unf, fus


def cg_init(b):
    """x = 0, r = p = b, p32 = float32(b), state = {b.b, 1}; also sum|b_i b_i|."""
    b = np.asarray(b, np.float64)
    bb, mag = dot(b, b)
    return dict(x=np.zeros_like(b), r=b.copy(), p=b.copy(), p32=b.astype(np.float32), state=np.array([bb, 1.0]),
                rr_abs=mag)


def cg_z(h, curv, damping, p, p32, A):
    """z = h + [curv * float64(p32) on the last A] + damping * p, and sum|addends| per element."""
    h, p = np.asarray(h, np.float64), np.asarray(p, np.float64)
    z, mag = h.copy(), np.abs(h)
    t = np.asarray(curv, np.float64) * np.asarray(p32, np.float32)[-A:].astype(np.float64)
    z[-A:] += t
    mag[-A:] += np.abs(t)
    z += np.float64(damping) * p
    mag += np.abs(np.float64(damping) * p)
    return z, mag


def cg_step(h, curv, damping, tol, x, r, p, p32, state, A):
    """One iteration of cg_solve.py's loop on z = f_Ax(p).  Returns a dict: z, zmag, pz, pz_abs, v,
    x, r, rr, rr_abs, mu, p, p32 and state = {r'.r', r'.r' < tol ? 0 : 1}.  A state with live == 0
    changes nothing: x, r, p, p32 come back as given and state = {state[0], 0}."""
    x, r, p = (np.asarray(v, np.float64) for v in (x, r, p))
    p32 = np.asarray(p32, np.float32)
    if state[1] == 0.0:
        return dict(x=x.copy(), r=r.copy(), p=p.copy(), p32=p32.copy(), state=np.array([state[0], 0.0]), live=False)
    z, zmag = cg_z(h, curv, damping, p, p32, A)
    pz, pz_abs = dot(p, z)
    v = div(state[0], pz)
    xn = x + v * p
    rn = r - v * z
    rr, rr_abs = dot(rn, rn)
    mu = div(rr, state[0])
    pn = rn + mu * p
    return dict(z=z, zmag=zmag, pz=pz, pz_abs=pz_abs, v=v, x=xn, r=rn, rr=rr, rr_abs=rr_abs, mu=mu, p=pn,
                p32=pn.astype(np.float32), state=np.array([rr, 0.0 if rr < tol else 1.0]), live=True)


def column_sums(partials):
    """(sum_b partials[b][c] rounded once, sum_b |partials[b][c]|) per column."""
    part = np.asarray(partials, np.float64)
    s = np.array([math.fsum(col) for col in part.T.tolist()])
    return s, np.abs(part).sum(0)


def ls_curvature(log_std_f32):
    """d^2 mean_kl / d log_std^2 at new == old per action: with s = exp(log_std)^2, the float64
    formula (8 s s - 4 s eps) / (2 s + eps)^2, eps = 1e-8, from exp evaluated in np.longdouble and
    rounded to float64.  Returns (curvature, magnitude): the magnitude is the same expression with
    the numerator's minus read as plus, the scale its rounding and exp's error act on."""
    ls = np.asarray(log_std_f32, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(ls.astype(np.longdouble)).astype(np.float64)
        sq, eps = e * e, 1e-8
        den = 2.0 * sq + eps
        return (8.0 * sq * sq - 4.0 * sq * eps) / (den * den), (8.0 * sq * sq + 4.0 * sq * eps) / (den * den)


def clamp_log_std(new32, min_ls, A):
    """torch.clamp(log_std, min_log_std) on the last A entries: NaN stays NaN."""
    out = np.array(new32, np.float32)
    tail = out[-A:]
    tail[tail < np.float32(min_ls)] = np.float32(min_ls)
    return out


def step_size(gdot, use_alpha, alpha, nss):
    """(alpha, n_step_size) of npg_cg.py:141-150 from gdot = vpg.npg."""
    if use_alpha:
        return float(alpha), float(np.float64(alpha) * np.float64(alpha) * np.float64(gdot))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(np.abs(np.float64(nss) / (np.float64(gdot) + 1e-20)))), float(nss)


def apply_step(vpg, npg, theta, use_alpha, alpha, nss, min_ls, A):
    """The step after the solve: gdot = vpg.npg; const_learn_rate (use_alpha): n_step_size =
    alpha^2 gdot, else alpha = sqrt(|n_step_size / (gdot + 1e-20)|); new = float32(float64(theta) +
    alpha npg) with the log_std block (the last A) clamped below at min_log_std.  Returns a dict:
    new, scal = {alpha, n_step_size, gdot}, gdot_abs."""
    vpg, npg = np.asarray(vpg, np.float64), np.asarray(npg, np.float64)
    theta = np.asarray(theta, np.float32)
    gdot, mag = dot(vpg, npg)
    al, ns = step_size(gdot, use_alpha, alpha, nss)
    with np.errstate(invalid="ignore", over="ignore"):
        new = (theta.astype(np.float64) + al * npg).astype(np.float32)
    return dict(new=clamp_log_std(new, min_ls, A), scal=np.array([al, ns, gdot]), gdot_abs=mag)
