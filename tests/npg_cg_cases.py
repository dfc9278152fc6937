"""The operands of tests/test_gpu_npg_cg.py and their reference results (numpy only, so that the
CPU suite can check that the exact operands are exact: tests/test_cpu_npg_cg_ref.py)."""
import numpy as np

import npg_cg_ref as C

U = 2.0 ** -53
RCC = 64  # columns per p.z part (k_npg_cg_reduce's second output)
SIZES = [(P, A) for P in (2, 63, 64, 65, 1023, 1024, 1025, 1154, 2048, 8616, 11456, 16383, 16384)
         for A in (1, 36, 64) if A < P] + [(65, 64), (1040, 36), (2064, 36)]
SIZES = sorted(set(SIZES))
_OPS, _REF = {}, {}


def operands(P, A, kind, nb=3):
    """p, r, x, p32, h, curv, damping, the [nb][P] partials whose column sums are h, state_in."""
    key = (P, A, kind, nb)
    if key in _OPS:
        return _OPS[key]
    rs = np.random.RandomState(P * 131 + A * 7 + nb)
    if kind == "exact":
        p = rs.randint(-8, 9, P).astype(np.float64)
        p[p == 0] = 3.0  # every element is felt by p.z and by the tail's curvature
        r = rs.randint(-8, 9, P).astype(np.float64)
        x = rs.randint(-8, 9, P).astype(np.float64)
        d = rs.randint(1, 5, P).astype(np.float64)
        curv = rs.randint(1, 13, A) / 4.0
        damping = 0.5 if (P + A) % 2 else 0.0
        h = d * p
        part = rs.randint(-64, 65, (nb, P)).astype(np.float64)
        part[nb - 1] = h - part[:nb - 1].sum(0)
    else:
        p, r, x = rs.randn(P), rs.randn(P), rs.randn(P)
        d = rs.uniform(0.5, 2.0, P)
        curv = C.ls_curvature((0.5 * rs.randn(A)).astype(np.float32))[0]
        damping = 1e-4
        w = rs.uniform(0.2, 1.0, (nb, P))
        part = w / w.sum(0) * (d * p)
        h = d * p
    p32 = p.astype(np.float32)
    o = dict(P=P, A=A, kind=kind, nb=nb, p=p, r=r, x=x, p32=p32, h=h, curv=curv, damping=damping, part=part)
    z, _ = C.cg_z(h, curv, damping, p, p32, A)
    pz = C.dot(p, z)[0]
    o["rdotr"] = pz / 8.0 if kind == "exact" else C.dot(r, r)[0]
    _OPS[key] = o
    return o


def reference(o, form, tol=0.0):
    """cg_step on the operands: from h itself for the step kernel, from the reference's column sums
    of the partials for the forms that reduce them.  Adds dh, the allowance on h."""
    key = (o["P"], o["A"], o["kind"], o["nb"], form == "step", tol)
    if key not in _REF:
        if form == "step":
            h, dh = o["h"], np.zeros(o["P"])
        else:
            h, mag = C.column_sums(o["part"])
            dh = (o["nb"] + 2) * U * mag
        ref = C.cg_step(h, o["curv"], o["damping"], tol, o["x"], o["r"], o["p"], o["p32"], [o["rdotr"], 1.0],
                        o["A"])
        ref["h"], ref["dh"] = h, dh
        _REF[key] = ref
    return _REF[key]


def parts_of(p, z):
    """p.z per 64 columns (k_npg_cg_reduce's second output), from the reference's dot."""
    return np.array([C.dot(p[i:i + RCC], z[i:i + RCC])[0] for i in range(0, p.size, RCC)])
