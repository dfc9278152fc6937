"""The solve half of csrc/amx_npg.hip -- k_npg_cg_init, k_npg_cg_step, k_npg_cg_reduce, k_npg_cg_xrp,
cg_fold at the head of k_npg, k_npg_curvature and k_npg_apply -- through the C ABI against the plain
reference tests/npg_cg_ref.py, at the sizes where each kernel's index arithmetic changes: P below,
on and above a 64-column reduce block and a 1024-element step block, the admitted maximum 16384,
A = 1 / 36 / 64 and tails that cross a block boundary, 1 to 256 partial blocks around the 16-block
run, a fold grid with more blocks than slices.

Every buffer a kernel writes starts as a sentinel and ends in a 256-element NaN fence that must
survive; whatever a kernel must not read (p32 before the log_std tail, every operand of a stopped
solve) holds NaN; in the stopped fold r_in and p_in are followed by a finite run, so that a slice
copied from past their end would show in the fence of the outputs.

Two kinds of operands.
EXACT: p, r, x and the partials are small integers, h = d * p with integer d >= 1, curv in k/4,
damping 0.5 or 0, p32 = float32(p), state_in[0] = p.z / 8 so that v = 1/8: z, p.z, x', r' and
r'.r' are each one real number in any summation order (tests/test_cpu_npg_cg_ref.py), and
the device must return them bit for bit; mu is then one correctly rounded division, and every
element of p' must be fl(r' + fl(mu p)) or the fused fl(r' + mu p) -- the test prints which.
REAL: randn p, r, x; h = d * p with d in [0.5, 2] (z has the sign of p: p.z has only positive
terms); curv from ls_curvature; damping 1e-4.  With u = 2^-53 and n = P the allowances are derived,
not measured.  A device sum is one fixed-order float64 sum of n <= 16384 non-negative terms: no
term passes more than n - 1 additions, its product rounds once, the reference's sum rounds once,
so |sum_dev - sum_ref| <= (n + 2) u sum|terms| given the same terms.  The terms themselves differ
where their inputs do, to first order:
  dz_i  = dh_i + 4 u (|h_i| + |curv p32| + |damping p_i|)      (two float64 evaluations of z;
          dh_i = (blocks + 2) u sum_b |partial_b,i| where h is a column sum, else 0)
  dpz   = (n + 2) u sum|p_i z_i| + sum |p_i| dz_i
  dv    = |v| (dpz / |p.z| + u)
  dx_i  = |p_i| dv + 2 u (|x_i| + 2 |v p_i|)
  dr_i  = |z_i| dv + |v| dz_i + 2 u (|r_i| + 2 |v z_i|)
  drr   = (n + 2) u sum r'_i^2 + sum 2 |r'_i| dr_i
  dmu   = drr / r.r + u mu
  dp_i  = dr_i + |p_i| dmu + 2 u (|r'_i| + 2 |mu p_i|)
and p32' must be float32 of the device's own p' bit for bit.  The live flag is asserted with tol
two allowances below and above the reference's r'.r'.  The same (n + 2) u sum|terms| holds b.b of
cg_init and vpg.npg of apply_step.

The curvature: the device's exp is taken to be within 1 ulp, i.e. e_dev = e (1 + d), |d| <= 2 u
against the reference's exp (np.longdouble, rounded).  s = e^2 carries 2 d, the numerator 8 s^2 -
4 s eps and the squared denominator (2 s + eps)^2 carry at most 4 d each on the scale of 8 s^2 +
4 s eps, the quotient 8 d = 16 u; the formula's ten float64 operations round once each on either
side, 20 u: |curv_dev - curv_ref| <= 36 u mag = 18 ulp of mag, mag being the formula with the
numerator's minus read as plus (no cancellation for s >> eps, where mag = |curv|).

Measured on an MI355X (largest |device - reference| / allowance; every exact case bit for bit,
every p' the unfused reading, as the library is built with -ffp-contract=off):
  step forms (step | tail | reduce + xrp): x 0.19 | 0.24 | 0.24, r' 0.18 | 0.44 | 0.58,
  p' 0.11 | 0.11 | 0.16, r'.r' 0.014 | 0.013 | 0.035; z 0.43, p.z parts 0.11; h of the reduction 0.26;
  b.b of cg_init 0.03; vpg.npg of apply_step 0.156; curvature 0.056 (one ulp of the value).
The file runs in 6 s (356 tests).
"""
import numpy as np
import pytest
import torch

import npg_cg_ref as C
from npg_cg_cases import RCC, SIZES, U, operands, parts_of, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
FENCE = 256
SENT = 7.0
NAN = float("nan")
PMAX, MAXB = 16384, 256
FORMS = ["step", "tail", "split"]
_CTX = {}


def ctx_for(S=11, A=3):
    import amp_extensions_amd as amx
    if (S, A) not in _CTX:
        _CTX[(S, A)] = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device=DEV)
    return _CTX[(S, A)]


def dev(a, dtype=np.float64):
    """A host array on the device, followed by the NaN fence."""
    a = np.ascontiguousarray(a, dtype)
    t = torch.full((a.size + FENCE,), NAN, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=DEV)
    t[:a.size] = torch.from_numpy(a.ravel()).to(DEV)
    return t


def sent(n, dtype=np.float64):
    return dev(np.full(n, SENT, dtype), dtype)


def host(t, n):
    """The first n elements, after checking that the fence behind them is intact."""
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert np.isnan(a[n:]).all(), "a kernel wrote past the end of a buffer"
    return a[:n]


def ok(c, rc):
    assert rc == 0, c.lib.amx_last_error().decode()


def eq(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def run(form, o, state, tol=0.0, poison=False):
    """One iteration in the given form from fresh buffers.  poison: every operand a stopped solve
    must not read is NaN.  Returns the outputs as numpy."""
    c = ctx_for()
    lib, P, A, nb = c.lib, o["P"], o["A"], o["nb"]
    nparts = (P + RCC - 1) // RCC
    p32_in = o["p32"].copy()
    p32_in[:P - A] = NAN  # only the log_std tail of p32 is an input
    x, r, p, p32 = dev(o["x"]), dev(o["r"]), dev(o["p"]), dev(p32_in, np.float32)
    fill = (lambda a: np.full_like(a, NAN)) if poison else (lambda a: a)
    curv, st = dev(fill(o["curv"])), dev(state)
    out = {}
    if form == "step":
        h = dev(fill(o["h"]))
        ok(c, lib.amx_npg_cg_step(c.h, P, A, h.data_ptr(), curv.data_ptr(), o["damping"], tol, x.data_ptr(),
                                  r.data_ptr(), p.data_ptr(), p32.data_ptr(), st.data_ptr(), c.stream))
        out.update(r=host(r, P), state=host(st, 2))
    else:
        part, r2, st2, work = dev(fill(o["part"])), sent(P), sent(2), sent(P + nparts)
        assert int(lib.amx_npg_cg_tail_work(P)) == P + nparts
        if form == "tail":
            ok(c, lib.amx_npg_cg_tail(c.h, part.data_ptr(), nb, P, A, curv.data_ptr(), o["damping"], tol,
                                      x.data_ptr(), r.data_ptr(), r2.data_ptr(), p.data_ptr(), p32.data_ptr(),
                                      st.data_ptr(), st2.data_ptr(), work.data_ptr(), c.stream))
        else:
            ok(c, lib.amx_npg_cg_reduce(c.h, part.data_ptr(), nb, P, A, curv.data_ptr(), o["damping"], p.data_ptr(),
                                        p32.data_ptr(), st.data_ptr(), work.data_ptr(), c.stream))
            out["p32_mid"] = host(p32, P).copy()
            ok(c, lib.amx_npg_cg_xrp(c.h, P, tol, x.data_ptr(), r.data_ptr(), r2.data_ptr(), p.data_ptr(),
                                     p32.data_ptr(), st.data_ptr(), st2.data_ptr(), work.data_ptr(), c.stream))
        eq(host(r, P), o["r"], "r_in was written")
        eq(host(st, 2), state, "state_in was written")
        out.update(r=host(r2, P), state=host(st2, 2), work=host(work, P + nparts))
    out.update(x=host(x, P), p=host(p, P), p32=host(p32, P), p32_in=p32_in)
    host(curv, A)
    return out


def check_p(got_p, got_p32, r_new, mu, p_old, tag):
    """p' per element is one of the two IEEE readings of r' + mu p; p32' the float32 of the one taken."""
    unf, fus = C.axpy_candidates(r_new, mu, p_old, got_p)
    is_u, is_f = got_p == unf, got_p == fus
    assert (is_u | is_f).all(), (tag, int((~(is_u | is_f)).sum()), "elements of p' are neither reading")
    eq(got_p32, got_p.astype(np.float32), "p32' is not float32(p')")
    print(f"P_PRIME {tag}: unfused-only {int((is_u & (unf != fus)).sum())} fused-only {int((is_f & ~is_u).sum())} "
          f"of {got_p.size}")


def check_exact(out, ref, o, form, tag):
    for k in ("x", "r", "state"):
        eq(out[k], ref[k], f"{tag} {k}")
    # mu is not an output: it is pinned through p', whose candidates take the reference's one division
    check_p(out["p"], out["p32"], ref["r"], ref["mu"], o["p"], tag)
    if form != "step":
        eq(out["work"][:o["P"]], ref["z"], f"{tag} zbuf")
        eq(out["work"][o["P"]:], parts_of(o["p"], ref["z"]), f"{tag} p.z parts")


def allowances(ref, o):
    """The docstring's first-order allowances for one step on real operands."""
    n, p, r, x = o["P"], np.abs(o["p"]), np.abs(o["r"]), np.abs(o["x"])
    z, v, mu = np.abs(ref["z"]), abs(ref["v"]), abs(ref["mu"])
    dz = ref["dh"] + 4 * U * ref["zmag"]
    dpz = (n + 2) * U * ref["pz_abs"] + float((p * dz).sum())
    dv = v * (dpz / abs(ref["pz"]) + U)
    dx = p * dv + 2 * U * (x + 2 * v * p)
    dr = z * dv + v * dz + 2 * U * (r + 2 * v * z)
    rn = np.abs(ref["r"])
    drr = (n + 2) * U * ref["rr_abs"] + float((2 * rn * dr).sum())
    dmu = drr / abs(o["rdotr"]) + U * mu
    dp = dr + p * dmu + 2 * U * (rn + 2 * mu * p)
    return dict(z=dz, pz=dpz, x=dx, r=dr, rr=drr, p=dp)


def check_real(out, ref, o, form, tag):
    al = allowances(ref, o)
    ratios = {k: float((np.abs(out[k] - ref[k]) / al[k]).max()) for k in ("x", "r", "p")}
    ratios["rr"] = abs(out["state"][0] - ref["rr"]) / al["rr"]
    if form != "step":
        P = o["P"]
        ratios["z"] = float((np.abs(out["work"][:P] - ref["z"]) / al["z"]).max())
        # each 64-column part: its own (64 + 2) u sum|terms| plus the propagated dz
        pp, pa = np.abs(o["p"]), np.abs(o["p"] * ref["z"])
        want = parts_of(o["p"], ref["z"])
        bound = np.array([(RCC + 2) * U * pa[i:i + RCC].sum() + (pp[i:i + RCC] * al["z"][i:i + RCC]).sum()
                          for i in range(0, P, RCC)])
        ratios["pz_part"] = float((np.abs(out["work"][P:] - want) / bound).max())
    eq(out["p32"], out["p"].astype(np.float32), "p32' is not float32(p')")
    print(f"RATIO cg {tag}: " + " ".join(f"{k}={v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (tag, ratios)
    return al


def check_stopped(out, o, s0, form, tag):
    """A stopped solve: x, p, p32 untouched, r carried over, state = {state_in[0], 0}, work untouched."""
    eq(out["x"], o["x"], f"{tag} x")
    eq(out["p"], o["p"], f"{tag} p")
    eq(out["p32"], out["p32_in"], f"{tag} p32")
    eq(out["r"], o["r"], f"{tag} r")
    eq(out["state"], [s0, 0.0], f"{tag} state")
    if form != "step":
        assert (out["work"] == SENT).all(), f"{tag}: work was written"


# ---- 1. amx_npg_cg_init / amx_npg_cg_init_ls ------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("P,A", SIZES)
def test_cg_init(P, A, kind):
    c = ctx_for()
    o = operands(P, A, kind)
    b = o["r"] * (1.0 if kind == "exact" else 1e3)
    ref = C.cg_init(b)
    theta = np.full(P, NAN, np.float32)  # the curvature reads theta[P - A ...] and nothing else
    ls = (0.5 * np.random.RandomState(P + A).randn(A)).astype(np.float32)
    theta[P - A:] = ls
    worst = 0.0
    for with_ls in (False, True):
        x, r, p, p32, st, curv = sent(P), sent(P), sent(P), sent(P, np.float32), sent(2), sent(A)
        bd, th = dev(b), dev(theta, np.float32)
        if with_ls:
            ok(c, c.lib.amx_npg_cg_init_ls(c.h, P, A, th.data_ptr(), curv.data_ptr(), bd.data_ptr(), x.data_ptr(),
                                           r.data_ptr(), p.data_ptr(), p32.data_ptr(), st.data_ptr(), c.stream))
            check_curvature(host(curv, A), ls, f"init_ls P={P} A={A}")
        else:
            ok(c, c.lib.amx_npg_cg_init(c.h, P, bd.data_ptr(), x.data_ptr(), r.data_ptr(), p.data_ptr(),
                                        p32.data_ptr(), st.data_ptr(), c.stream))
            assert (host(curv, A) == SENT).all()
        for k, t in (("x", x), ("r", r), ("p", p), ("p32", p32)):
            eq(host(t, P), ref[k], k)
        s = host(st, 2)
        assert s[1] == 1.0
        if kind == "exact":
            assert s[0] == ref["state"][0]
        else:
            worst = max(worst, abs(s[0] - ref["state"][0]) / ((P + 2) * U * ref["rr_abs"]))
    if kind == "real":
        print(f"RATIO init P={P} A={A}: bb={worst:.4f}")
        assert worst <= 1.0


# ---- 2. the step in its three forms ---------------------------------------------------------
@pytest.mark.parametrize("P,A", SIZES)
def test_cg_step_exact(P, A):
    """Live: the reference bit for bit in all three forms, with tol one ulp below r'.r' (flag 1),
    equal to it (flag 1) and one ulp above (flag 0); tail == reduce + xrp follows."""
    o = operands(P, A, "exact")
    state = [o["rdotr"], 1.0]
    outs = {}
    for form in FORMS:
        rr = reference(o, form)["rr"]
        for tol, live in ((np.nextafter(rr, 0.0), 1.0), (rr, 1.0), (np.nextafter(rr, np.inf), 0.0)):
            ref = dict(reference(o, form), state=np.array([rr, live]))
            out = run(form, o, state, tol=float(tol))
            check_exact(out, ref, o, form, f"{form} P={P} A={A} tol={'<=>'[int(np.sign(tol - rr)) + 1]}rr")
        outs[form] = out
    for k in ("x", "r", "p", "p32", "state", "work"):
        eq(outs["tail"][k], outs["split"][k], f"tail vs reduce + xrp: {k}")


@pytest.mark.parametrize("P,A", SIZES)
def test_cg_step_real(P, A):
    o = operands(P, A, "real")
    state = [o["rdotr"], 1.0]
    outs = {}
    for form in FORMS:
        ref = reference(o, form)
        outs[form] = out = run(form, o, state)
        al = check_real(out, ref, o, form, f"{form} P={P} A={A}")
        assert out["state"][1] == 1.0
        for tol, live in ((ref["rr"] - 2 * al["rr"], 1.0), (ref["rr"] + 2 * al["rr"], 0.0)):
            assert run(form, o, state, tol=tol)["state"][1] == live, (form, tol)
    for k in ("x", "r", "p", "p32", "state", "work"):
        eq(outs["tail"][k], outs["split"][k], f"tail vs reduce + xrp: {k}")


@pytest.mark.parametrize("P,A", SIZES)
def test_cg_step_stopped(P, A):
    o = operands(P, A, "exact")
    for form in FORMS:
        out = run(form, o, [o["rdotr"], 0.0], tol=1e300, poison=True)
        check_stopped(out, o, o["rdotr"], form, f"{form} P={P} A={A}")


# ---- 3. the reduction over 1 to 256 partial blocks ------------------------------------------
BLOCKS = [1, 15, 16, 17, 32, 33, 255, 256]
REDUCE_CASES = [(65, A, nb) for A in (1, 36, 64) for nb in BLOCKS] + \
               [(1025, 36, nb) for nb in BLOCKS] + [(8616, 36, nb) for nb in (1, 16, 17, 256)] + [(16384, 64, 256)]


def device_h(c, part, nb, P):
    out = sent(P)
    ok(c, c.lib.amx_npg_reduce(c.h, part.data_ptr(), nb, P, out.data_ptr(), c.stream))
    return host(out, P)


@pytest.mark.parametrize("P,A,nb", REDUCE_CASES)
def test_cg_reduce_blocks_exact(P, A, nb):
    o = operands(P, A, "exact", nb)
    for form in ("tail", "split"):
        out = run(form, o, [o["rdotr"], 1.0])
        check_exact(out, reference(o, form), o, form, f"{form} P={P} A={A} blocks={nb}")


@pytest.mark.parametrize("P,A,nb", [c for c in REDUCE_CASES if c[0] < PMAX])
def test_cg_reduce_blocks_real(P, A, nb):
    """The step on the column sums of real partials inside the allowances, and h itself -- zbuf
    under zero curvature and damping -- equal to amx_npg_reduce's output bit for bit."""
    c = ctx_for()
    o = operands(P, A, "real", nb)
    ref = reference(o, "split")
    check_real(run("split", o, [o["rdotr"], 1.0]), ref, o, "split", f"split P={P} A={A} blocks={nb}")
    part = dev(o["part"])
    h_dev = device_h(c, part, nb, P)
    r = float((np.abs(h_dev - ref["h"]) / ref["dh"]).max())
    print(f"RATIO reduce P={P} blocks={nb}: h={r:.4f}")
    assert r <= 1.0
    o0 = dict(o, curv=np.zeros(A), damping=0.0)
    eq(run("split", o0, [o["rdotr"], 1.0])["work"][:P], h_dev, "k_npg_cg_reduce's h is not amx_npg_reduce's")


# ---- 4. refusals ----------------------------------------------------------------------------
def test_refusals():
    """Return code -1, the entry point's name in amx_last_error, nothing written."""
    c = ctx_for()
    lib, P, A = c.lib, 1025, 36
    b = {k: sent(PMAX + 1) for k in ("part", "x", "r", "r2", "p", "h", "vpg", "npg", "work")}
    b.update(p32=sent(PMAX + 1, np.float32), theta=sent(PMAX + 1, np.float32), new=sent(PMAX + 1, np.float32),
             st=dev([1.0, 1.0]), st2=sent(2), curv=sent(PMAX + 1), scal=sent(3))
    q = {k: t.data_ptr() for k, t in b.items()}

    def tail(P=P, A=A, nb=3, r2="r2", st2="st2"):
        return lib.amx_npg_cg_tail(c.h, q["part"], nb, P, A, q["curv"], 0.0, 0.0, q["x"], q["r"], q[r2], q["p"],
                                   q["p32"], q["st"], q[st2], q["work"], c.stream)

    def reduce(P=P, A=A, nb=3):
        return lib.amx_npg_cg_reduce(c.h, q["part"], nb, P, A, q["curv"], 0.0, q["p"], q["p32"], q["st"], q["work"],
                                     c.stream)

    def xrp(P=P, r2="r2", st2="st2"):
        return lib.amx_npg_cg_xrp(c.h, P, 0.0, q["x"], q["r"], q[r2], q["p"], q["p32"], q["st"], q[st2], q["work"],
                                  c.stream)

    def step(P=P, A=A):
        return lib.amx_npg_cg_step(c.h, P, A, q["h"], q["curv"], 0.0, 0.0, q["x"], q["r"], q["p"], q["p32"], q["st2"],
                                   c.stream)

    def init(P=P):
        return lib.amx_npg_cg_init(c.h, P, q["h"], q["x"], q["r"], q["p"], q["p32"], q["st2"], c.stream)

    def init_ls(P=P, A=A):
        return lib.amx_npg_cg_init_ls(c.h, P, A, q["theta"], q["curv"], q["h"], q["x"], q["r"], q["p"], q["p32"],
                                      q["st2"], c.stream)

    def curvature(P=P, A=A):
        return lib.amx_npg_curvature(c.h, q["theta"], P, A, q["curv"], c.stream)

    def apply(P=P, A=A):
        return lib.amx_npg_apply_step(c.h, P, A, q["vpg"], q["npg"], q["theta"], 0, 0.0, 0.1, -2.0, q["new"],
                                      q["scal"], c.stream)

    cases = [("amx_npg_cg_tail", tail, [dict(nb=0), dict(nb=MAXB + 1), dict(P=PMAX + 1), dict(A=0), dict(A=P),
                                        dict(r2="r"), dict(st2="st")]),
             ("amx_npg_cg_reduce", reduce, [dict(nb=0), dict(nb=MAXB + 1), dict(P=PMAX + 1), dict(A=0), dict(A=P)]),
             ("amx_npg_cg_xrp", xrp, [dict(P=PMAX + 1), dict(P=0), dict(r2="r"), dict(st2="st")]),
             ("amx_npg_cg_step", step, [dict(P=PMAX + 1), dict(A=0)]),
             ("amx_npg_cg_init", init, [dict(P=PMAX + 1), dict(P=0)]),
             ("amx_npg_cg_init_ls", init_ls, [dict(P=PMAX + 1), dict(A=0), dict(A=P)]),
             ("amx_npg_curvature", curvature, [dict(A=0), dict(A=P)]),
             ("amx_npg_apply_step", apply, [dict(P=PMAX + 1), dict(A=0), dict(A=P)])]
    for name, fn, bad in cases:
        for kw in bad:
            assert fn(**kw) == -1, (name, kw)
            assert name in lib.amx_last_error().decode(), (name, kw, lib.amx_last_error().decode())
    for k, t in b.items():
        if k != "st":
            assert (host(t, t.numel() - FENCE) == SENT).all(), f"a refused call wrote {k}"


# ---- 5. amx_npg_curvature -------------------------------------------------------------------
LS_VALUES = np.array([-20.0, -2.0, -0.25, 0.0, 0.5, 2.0, 40.0, 88.0, NAN], np.float32)


def check_curvature(got, ls, tag):
    want, mag = C.ls_curvature(ls)
    nan = np.isnan(ls)
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), tag
    ratio = float((np.abs(got[~nan] - want[~nan]) / (36 * U * mag[~nan])).max()) if (~nan).any() else 0.0
    print(f"RATIO curvature {tag}: {ratio:.4f}")
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("A", [1, 63, 64, 65])
@pytest.mark.parametrize("via", ["curvature", "init_ls"])
def test_curvature(A, via):
    """The named values (rotated so that A = 1 sees each) and randn, read from theta[P - A ...]
    behind a NaN front.  amx_npg_curvature has no bound on A (one 64-thread block per 64 actions):
    A = 65 is admitted there too, and tested."""
    c = ctx_for()
    rs = np.random.RandomState(A)
    for rot in range(LS_VALUES.size if A == 1 else 2):
        ls = np.concatenate([np.roll(LS_VALUES, -rot), rs.randn(max(A, 9)).astype(np.float32)])[:A]
        if A > 9 and rot:
            ls = ls[::-1].copy()
        P = A + 70
        theta = np.full(P, NAN, np.float32)
        theta[P - A:] = ls
        th, curv = dev(theta, np.float32), sent(A)
        if via == "curvature":
            ok(c, c.lib.amx_npg_curvature(c.h, th.data_ptr(), P, A, curv.data_ptr(), c.stream))
        else:
            t = [dev(np.ones(P))] + [sent(P) for _ in range(3)] + [sent(P, np.float32), sent(2)]
            ok(c, c.lib.amx_npg_cg_init_ls(c.h, P, A, th.data_ptr(), curv.data_ptr(), *[v.data_ptr() for v in t],
                                           c.stream))
        check_curvature(host(curv, A), ls, f"{via} A={A} rot={rot}")


# ---- 6. amx_npg_apply_step ------------------------------------------------------------------
APPLY_SIZES = [(P, A) for P in (2, 1024, 1025, 8616, 16384) for A in (1, 36, 64) if A < P]
MIN_LS = np.float32(-2.0)


def run_apply(P, A, vpg, npg, theta, use_alpha, alpha, nss):
    c = ctx_for()
    new, scal = sent(P, np.float32), sent(3)
    v, n, th = dev(vpg), dev(npg), dev(theta, np.float32)
    ok(c, c.lib.amx_npg_apply_step(c.h, P, A, v.data_ptr(), n.data_ptr(), th.data_ptr(), use_alpha, alpha, nss,
                                   float(MIN_LS), new.data_ptr(), scal.data_ptr(), c.stream))
    out = host(new, P), host(scal, 3)
    eq(host(th, P), theta, "theta was written")
    return out


def check_new(new, theta, npg, alpha, A, tag):
    """new = float32(float64(theta) + alpha npg) in one of the two IEEE readings, given the device's
    own alpha, then the clamp on exactly the last A."""
    unf, fus = C.axpy_candidates(theta.astype(np.float64), alpha, npg, new.astype(np.float64), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        cu, cf = (C.clamp_log_std(v.astype(np.float32), MIN_LS, A) for v in (unf, fus))
    same = lambda a, b: (a == b) | (np.isnan(a) & np.isnan(b))
    is_u, is_f = same(new, cu), same(new, cf)
    assert (is_u | is_f).all(), (tag, np.nonzero(~(is_u | is_f))[0][:8])
    return int((is_f & ~is_u).sum())


@pytest.mark.parametrize("P,A", APPLY_SIZES)
def test_apply_step_exact(P, A):
    """Integer vpg / npg: gdot exact, positive, negative and exactly 0, in both step-size modes;
    scal bit for bit (alpha one division and one square root, both correctly rounded; at gdot = 0
    the 1e-20 guard gives sqrt(nss * 1e20))."""
    rs = np.random.RandomState(P + A)
    npg = rs.randint(-8, 9, P).astype(np.float64)
    vpg = rs.randint(-8, 9, P).astype(np.float64)
    vpg[0], npg[0] = 1.0, 1.0
    theta = rs.randn(P).astype(np.float32)
    g0 = float(vpg @ npg)
    fused = 0
    for sign in (1, -1, 0):
        v = vpg.copy()
        n = npg.copy()
        if sign == 0:
            n[0] -= g0
        elif np.sign(g0) != sign:
            v = -v if g0 != 0 else v
            if g0 == 0:
                n[0] += sign
        want_g = float(v @ n)
        assert np.sign(want_g) == sign
        for use_alpha in (0, 1):
            ref = C.apply_step(v, n, theta, use_alpha, 0.25, 0.1, MIN_LS, A)
            assert ref["scal"][2] == want_g
            new, scal = run_apply(P, A, v, n, theta, use_alpha, 0.25 if use_alpha else NAN, NAN if use_alpha else 0.1)
            eq(scal, ref["scal"], f"scal sign={sign} use_alpha={use_alpha}")
            if sign == 0 and not use_alpha:
                assert scal[0] == np.sqrt(0.1 / 1e-20)
            fused += check_new(new, theta, n, scal[0], A, f"P={P} A={A} sign={sign} use_alpha={use_alpha}")
    print(f"APPLY P={P} A={A}: fused-only elements {fused}")


@pytest.mark.parametrize("P,A", APPLY_SIZES)
def test_apply_step_real(P, A):
    rs = np.random.RandomState(P * 3 + A)
    vpg, npg = rs.randn(P), rs.randn(P)
    theta = rs.randn(P).astype(np.float32)
    worst = 0.0
    for sgn in (1.0, -1.0):
        for use_alpha in (0, 1):
            ref = C.apply_step(sgn * vpg, npg * vpg ** 2, theta, use_alpha, 0.25, 0.1, MIN_LS, A)
            new, scal = run_apply(P, A, sgn * vpg, npg * vpg ** 2, theta, use_alpha, 0.25, 0.1)
            dg = (P + 2) * U * ref["gdot_abs"]
            worst = max(worst, abs(scal[2] - ref["scal"][2]) / dg)
            al, ns = C.step_size(scal[2], use_alpha, 0.25, 0.1)  # from the device's own gdot: bit for bit
            eq(scal[:2], [al, ns])
            check_new(new, theta, npg * vpg ** 2, scal[0], A, f"P={P} A={A}")
    print(f"RATIO apply P={P} A={A}: gdot={worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("P,A", APPLY_SIZES)
def test_apply_step_clamp(P, A):
    """npg = 0 where the value is planted, so new = theta there: one float32 ulp below min_log_std
    (clamped), equal to it and one ulp above (kept), NaN (kept) at the first element of the log_std
    block -- e = P - A -- and at its last; element P - A - 1, far below, is left alone."""
    rs = np.random.RandomState(P + 5 * A)
    below, above = np.nextafter(MIN_LS, np.float32(-np.inf)), np.nextafter(MIN_LS, np.float32(np.inf))
    for val, want in ((below, MIN_LS), (MIN_LS, MIN_LS), (above, above), (np.float32(NAN), np.float32(NAN)),
                      (np.float32(-1e30), MIN_LS)):
        vpg, npg = rs.randint(1, 9, P).astype(np.float64), rs.randint(1, 9, P).astype(np.float64)
        theta = (rs.randn(P) - 9.0).astype(np.float32)  # every clamped slot would change
        spots = {P - A: val, P - 1: val}
        for e, v in spots.items():
            theta[e], npg[e] = v, 0.0
        if P - A - 1 >= 0:
            theta[P - A - 1], npg[P - A - 1] = np.float32(-100.0), 0.0
        new, scal = run_apply(P, A, vpg, npg, theta, 1, 2.0 ** -10, NAN)
        ref = C.apply_step(vpg, npg, theta, 1, 2.0 ** -10, NAN, MIN_LS, A)
        eq(scal, ref["scal"])
        check_new(new, theta, npg, scal[0], A, f"clamp P={P} A={A} val={val}")
        for e in spots:
            assert new[e] == want or (np.isnan(want) and np.isnan(new[e])), (e, val, new[e])
        if P - A - 1 >= 0:
            assert new[P - A - 1] == np.float32(-100.0)
            assert (new[:P - A] < MIN_LS).all()  # nothing before the block is clamped
        assert not (new[P - A:] < MIN_LS).any()


# ---- 7. the fold (amx_npg_pass_cg, amx_npg_pass_cg_idx) --------------------------------------
FOLD_SHAPES = [(1, 1), (11, 3), (197, 36), (256, 64)]
FOLD_GRIDS = [(20, 32), (40, 32), (8192, 32)]  # (N, rows_per_block): 1, 2 and 256 blocks
_FOLD = {}


def fold_inputs(S, A, N):
    key = (S, A, N)
    if key not in _FOLD:
        from amp_extensions_amd.policy import init_mlp_policy_params
        from amp_extensions_amd.npg import pack_policy
        layers, ls = init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25)
        rs = np.random.RandomState(S + N)
        obs = torch.from_numpy((0.5 * rs.randn(N, S)).astype(np.float32)).to(DEV)
        idx = rs.permutation(N).astype(np.int32)
        idx[: N // 4] = idx[N // 2]  # duplicates
        _FOLD[key] = (torch.from_numpy(pack_policy(layers, ls)).to(DEV), obs,
                      torch.zeros(N, A, dtype=torch.float32, device=DEV), torch.from_numpy(idx).to(DEV))
    return _FOLD[key]


def fvp(c, theta, obs, act, vec, rpb, part, gate=None, idx=None):
    N = obs.shape[0]
    if idx is None:
        ok(c, c.lib.amx_npg_pass_ex(c.h, 1, N, obs.data_ptr(), 1, obs.stride(0), act.data_ptr(), 1, act.stride(0),
                                    None, theta.data_ptr(), vec.data_ptr(), rpb, part.data_ptr(),
                                    None if gate is None else gate.data_ptr(), None, c.stream))
    else:
        ok(c, c.lib.amx_npg_pass_idx(c.h, N, N, idx.data_ptr(), obs.data_ptr(), 1, obs.stride(0), theta.data_ptr(),
                                     vec.data_ptr(), rpb, part.data_ptr(), None if gate is None else gate.data_ptr(),
                                     None, None, c.stream))


def fold(c, *args, **kw):
    ok(c, fold_rc(c, *args, **kw))


def fold_rc(c, theta, obs, rpb, part, tol, x, r, r2, p, p2, p32b, st, st2, work, idx=None):
    N = obs.shape[0]
    args = (obs.data_ptr(), 1, obs.stride(0), theta.data_ptr(), rpb, part.data_ptr(), None, tol, x.data_ptr(),
            r.data_ptr(), r2.data_ptr(), p.data_ptr(), p2.data_ptr(), p32b.data_ptr(), st.data_ptr(), st2.data_ptr(),
            work.data_ptr())
    if idx is None:
        return c.lib.amx_npg_pass_cg(c.h, N, *args, c.stream)
    return c.lib.amx_npg_pass_cg_idx(c.h, N, N, idx.data_ptr(), *args, None, c.stream)


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "idx"])
def test_fold_refusals(indexed):
    """r, p and the state must alternate buffers in the fold too: -1, the entry point named, nothing
    written."""
    S, A, N = 11, 3, 40
    c = ctx_for(S, A)
    theta, obs, _, idx = fold_inputs(S, A, N)
    P = int(c.lib.amx_npg_param_count(S, A))
    t = {k: sent(P) for k in ("x", "r", "r2", "p", "p2", "work")}
    t.update(p32b=sent(P, np.float32), st=dev([1.0, 1.0]), st2=sent(2), part=sent(2 * P))
    for swap in (dict(r2="r"), dict(p2="p"), dict(st2="st")):
        n = dict({k: k for k in t}, **swap)
        rc = fold_rc(c, theta, obs, 32, t["part"], 0.0, t["x"], t["r"], t[n["r2"]], t["p"], t[n["p2"]], t["p32b"],
                     t["st"], t[n["st2"]], t["work"], idx=idx if indexed else None)
        assert rc == -1, swap
        assert ("amx_npg_pass_cg_idx:" if indexed else "amx_npg_pass_cg:") in c.lib.amx_last_error().decode()
    for k, v in t.items():
        if k != "st":
            assert (host(v, v.numel() - FENCE) == SENT).all(), f"a refused fold wrote {k}"


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("N,rpb", FOLD_GRIDS)
@pytest.mark.parametrize("S,A", FOLD_SHAPES)
def test_fold_matches_tail_form(S, A, N, rpb, indexed):
    """One and three iterations of the solve with the vector step folded into the next pass against
    the pass + amx_npg_cg_tail form: x, r, p, p32 and the state bit for bit."""
    c = ctx_for(S, A)
    lib = c.lib
    theta, obs, act, idx = fold_inputs(S, A, N)
    idx = idx if indexed else None
    P = int(lib.amx_npg_param_count(S, A))
    nb, nparts, damping = (N + rpb - 1) // rpb, (P + RCC - 1) // RCC, 1e-4
    b = dev(np.random.RandomState(P).randn(P))

    def start():
        t = dict(x=sent(P), r=sent(P), p=sent(P), p32=sent(P, np.float32), st=sent(2), curv=sent(A), r2=sent(P),
                 p2=sent(P), p32b=sent(P, np.float32), st2=sent(2), work=sent(P + nparts), part=sent(nb * P))
        ok(c, lib.amx_npg_cg_init_ls(c.h, P, A, theta.data_ptr(), t["curv"].data_ptr(), b.data_ptr(),
                                     t["x"].data_ptr(), t["r"].data_ptr(), t["p"].data_ptr(), t["p32"].data_ptr(),
                                     t["st"].data_ptr(), c.stream))
        return t

    def result(t):
        return [host(t[k], n).copy() for k, n in (("x", P), ("r", P), ("p", P), ("p32", P), ("st", 2))]

    for iters in (1, 3):
        t = start()
        for _ in range(iters):
            fvp(c, theta, obs, act, t["p32"], rpb, t["part"], gate=t["st"], idx=idx)
            ok(c, lib.amx_npg_cg_tail(c.h, t["part"].data_ptr(), nb, P, A, t["curv"].data_ptr(), damping, 0.0,
                                      t["x"].data_ptr(), t["r"].data_ptr(), t["r2"].data_ptr(), t["p"].data_ptr(),
                                      t["p32"].data_ptr(), t["st"].data_ptr(), t["st2"].data_ptr(),
                                      t["work"].data_ptr(), c.stream))
            t["r"], t["r2"], t["st"], t["st2"] = t["r2"], t["r"], t["st2"], t["st"]
        want = result(t)
        host(t["part"], nb * P), host(t["work"], P + nparts)
        t = start()
        for it in range(iters):
            if it == 0:
                fvp(c, theta, obs, act, t["p32"], rpb, t["part"], gate=t["st"], idx=idx)
            else:
                fold(c, theta, obs, rpb, t["part"], 0.0, t["x"], t["r"], t["r2"], t["p"], t["p2"], t["p32b"], t["st"],
                     t["st2"], t["work"], idx=idx)
                for u, v in (("r", "r2"), ("p", "p2"), ("p32", "p32b"), ("st", "st2")):
                    t[u], t[v] = t[v], t[u]
            ok(c, lib.amx_npg_cg_reduce(c.h, t["part"].data_ptr(), nb, P, A, t["curv"].data_ptr(), damping,
                                        t["p"].data_ptr(), t["p32"].data_ptr(), t["st"].data_ptr(),
                                        t["work"].data_ptr(), c.stream))
        ok(c, lib.amx_npg_cg_xrp(c.h, P, 0.0, t["x"].data_ptr(), t["r"].data_ptr(), t["r2"].data_ptr(),
                                 t["p"].data_ptr(), t["p32"].data_ptr(), t["st"].data_ptr(), t["st2"].data_ptr(),
                                 t["work"].data_ptr(), c.stream))
        t["r"], t["st"] = t["r2"], t["st2"]
        got = result(t)
        for k in ("r2", "p2", "p32b", "st2", "part", "work", "curv"):
            host(t[k], t[k].numel() - FENCE)
        assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0 and want[4][1] == 1.0
        for name, u, v in zip(("x", "r", "p", "p32", "state"), want, got):
            eq(v, u, f"{name} after {iters} iterations")


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("N,rpb", FOLD_GRIDS)
@pytest.mark.parametrize("S,A", FOLD_SHAPES)
def test_fold_first_step_exact_and_stopped(S, A, N, rpb, indexed):
    """The folded step from an exact-operand state (z and the p.z parts written by the host): the
    reference bit for bit, with tol on either side of r'.r'; its product is the plain pass on the
    p32' it wrote.  A stopped fold carries r and p over, leaves x alone and writes no partial."""
    c = ctx_for(S, A)
    theta, obs, act, idx = fold_inputs(S, A, N)
    idx = idx if indexed else None
    P = int(c.lib.amx_npg_param_count(S, A))
    nb, nparts = (N + rpb - 1) // rpb, (P + RCC - 1) // RCC
    o = operands(P, A, "exact")
    ref0 = reference(o, "step")
    work_h = np.concatenate([ref0["z"], parts_of(o["p"], ref0["z"])])
    rr = ref0["rr"]
    for tol, live in ((float(np.nextafter(rr, 0.0)), 1.0), (float(np.nextafter(rr, np.inf)), 0.0), (None, 0.0)):
        stopped = tol is None
        # r_in and p_in are followed by a finite run before their fence: a slice that ran past P would
        # carry it into the fence of r_out / p_out / p32_out (NaN copied onto NaN would not show)
        pad = np.full(FENCE, 5.0)
        x, st = dev(o["x"]), dev([o["rdotr"], 0.0 if stopped else 1.0])
        r, p = dev(np.concatenate([o["r"], pad])), dev(np.concatenate([o["p"], pad]))
        r2, p2, p32b, st2, part = sent(P), sent(P), sent(P, np.float32), sent(2), sent(nb * P)
        work = dev(np.full(P + nparts, NAN) if stopped else work_h)
        fold(c, theta, obs, rpb, part, 1e300 if stopped else tol, x, r, r2, p, p2, p32b, st, st2, work, idx=idx)
        eq(host(r, P + FENCE)[:P], o["r"], "r_in was written")
        eq(host(p, P + FENCE)[:P], o["p"], "p_in was written")
        got = dict(x=host(x, P), r=host(r2, P), p=host(p2, P), p32=host(p32b, P), state=host(st2, 2))
        tag = f"fold S={S} A={A} N={N} {'idx' if indexed else 'rows'}"
        if stopped:
            eq(got["x"], o["x"]), eq(got["r"], o["r"]), eq(got["p"], o["p"])
            eq(got["p32"], o["p32"]), eq(got["state"], [o["rdotr"], 0.0])
            assert (host(part, nb * P) == SENT).all(), "a stopped fold wrote a partial"
            continue
        check_exact(got, dict(ref0, state=np.array([rr, live])), o, "step", f"{tag} live={live}")
        pt = host(part, nb * P).copy()
        if live:
            want = sent(nb * P)
            fvp(c, theta, obs, act, p32b, rpb, want, idx=idx)
            eq(pt, host(want, nb * P), "the fold's product is not the plain pass on p32'")
        else:
            assert (pt == SENT).all(), "a fold that stopped the solve wrote a partial"
