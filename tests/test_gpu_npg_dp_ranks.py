"""The data-parallel NPG update over two ranks (fresh processes, gloo over host copies, one shared
card; tests/npg_dp_worker.py) against one process over the union of their rows.

The two worker processes run the four cases one after another in one process group (started once
for the module), so a rank that left a case one collective ahead of or behind the other would make
the next case hang (the communicate timeout) or mismatch.

Exact case.  512 + 512 rows at 32 rows per block are 16 blocks per rank: one run of the reduce's
first stage each, and the union's 32 blocks are the same two runs (k_npg_reduce1 / k_npg_cg_reduce
sum runs of RB = 16 consecutive blocks, then the runs in order from 0.0).  A rank's message is its
run sum, the two-term all-reduce one commutative add, and 0.0 + (run0 + run1) are the bits of
(0.0 + run0) + run1: theta, vpg_grad, npg_grad and alpha equal the union's bit for bit.

Uneven case.  200 + 549 rows cut the union's blocks elsewhere (another summation tree), so the
ranks' update is judged as the parent's single-process update is: against an fp64 restatement of
the update over the union (npg_pass_ref's passes, a numpy CG after mjrl's cg_solve with the tangent
cast to fp32 as the reference's HVP casts it, the step and the log_std clamp), in the 2-norm --
theta against the restatement's unrounded fp64 parameters, so the fp32 rounding of the stored
parameters is in both errors alike -- and must stay within 2 x the single-process error.
Measured on an MI355X (data-parallel | single process; the test prints them as DP_ERR):
theta 1.102e-03 | 9.804e-04, npg_grad 5.369e-03 | 4.929e-03 (|npg_grad| = 9.345),
kl_dist 1.059e-05 | 6.678e-06 (kl_dist = 2.501e-02).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import npg_pass_ref as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S, A = 197, 36


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("npg_dp")
    port = _free_port()
    outs = [str(tmp / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "npg_dp_worker.py"), str(r), "2", str(port),
                               outs[r]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=240)
            logs.append(o.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-4000:]
    return [dict(np.load(o)) for o in outs]


def union_update(n, whiten):
    """The parent's single-process update over the union's rows, in this process."""
    import torch

    import amp_extensions_amd as amx
    import npg_dp_worker as W
    from amp_extensions_amd.npg import unpack_policy
    d = P.inputs(S, A, n)
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device="cuda")
    layers, ls = unpack_policy(d["theta"], S, A)
    npg = amx.DeviceNPG(ctx, layers, ls, **W.NPG_ARGS)
    o = npg.train_from_arrays(d["obs"], d["act"], d["adv"], whiten=whiten)
    torch.cuda.synchronize()
    return dict(theta=npg.theta.cpu().numpy(), vpg=o["vpg_grad"].cpu().numpy(), npg=o["npg_grad"].cpu().numpy(),
                adv=o["advantages"].cpu().numpy(),
                scal=np.array([o["alpha"], o["delta"], o["surr_after"], o["kl_dist"]]))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


GLOBALS = ("theta", "vpg", "npg", "scal")


def test_refused_option_before_any_collective(ranks):
    for r in ranks:
        assert str(r["refused_error"]).startswith("NotImplementedError") and "BC term" in str(r["refused_error"])
        assert int(r["refused_calls"]) == 0


def test_empty_rank_same_error_on_both(ranks):
    errs = [str(r["empty_error"]) for r in ranks]
    assert errs[0] == errs[1] and errs[0].startswith("ValueError") and "rank 0" in errs[0]
    for r in ranks:  # the count exchange and nothing after it
        assert r["empty_calls"].tolist() == [2]


def test_exact_case_equals_the_union(ranks):
    Pn = P.param_count(S, A)
    one = union_update(1024, whiten=False)
    for r in ranks:
        assert str(r["exact_error"]) == "" and int(r["exact_n_total"]) == 1024
        assert r["exact_calls"].tolist() == [2] + [Pn] * 11 + [2]
    for k in GLOBALS:
        assert same(ranks[0][f"exact_{k}"], ranks[1][f"exact_{k}"]), k
    for k in ("theta", "vpg", "npg"):
        assert same(ranks[0][f"exact_{k}"], one[k]), (k, float(np.abs(ranks[0][f"exact_{k}"] - one[k]).max()))
    assert same(ranks[0]["exact_scal"][:2], one["scal"][:2])  # alpha, delta
    assert np.isfinite(one["theta"]).all() and not same(one["theta"], P.inputs(S, A, 1024)["theta"])
    # each rank's own rows (not whitened here)
    adv = P.inputs(S, A, 1024)["adv"]
    assert same(ranks[0]["exact_adv"], adv[:512]) and same(ranks[1]["exact_adv"], adv[512:])


def restated_update(n, nss=0.05, min_ls=-2.0, iters=10, damping=1e-4, tol=1e-10):
    """The whitened update over the union in fp64 numpy: (unrounded new parameters, npg_grad, kl)."""
    d = P.inputs(S, A, n)
    th = d["theta"]
    adv = (d["adv"] - d["adv"].mean()) / (d["adv"].std() + 1e-6)
    b = P.pass_ref(P.VPG, S, A, th, d["obs"], d["act"], adv, None)[0]
    s = np.exp(th[-A:].astype(np.float64)) ** 2
    curv = (8.0 * s * s - 4.0 * s * 1e-8) / (2.0 * s + 1e-8) ** 2

    def hvp(v):
        v32 = v.astype(np.float32)
        h = P.pass_ref(P.FVP, S, A, th, d["obs"], d["act"], None, v32)[0]
        h[-A:] += curv * v32[-A:].astype(np.float64)
        return h + damping * v
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rdotr = r @ r
    for _ in range(iters):  # mjrl/mjrl/utils/cg_solve.py
        z = hvp(p)
        v = rdotr / (p @ z)
        x += v * p
        r -= v * z
        new = r @ r
        p = r + (new / rdotr) * p
        rdotr = new
        if rdotr < tol:
            break
    alpha = np.sqrt(np.abs(nss / (b @ x + 1e-20)))
    new = th.astype(np.float64) + alpha * x
    new[-A:] = np.maximum(new[-A:], min_ls)
    kl = P.pass_ref(P.EVAL, S, A, th, d["obs"], d["act"], adv, new.astype(np.float32))[0][1] / n
    return new, x, kl, adv


def test_uneven_case_with_whitening(ranks):
    n = 749
    for r in ranks:
        assert str(r["uneven_error"]) == "" and int(r["uneven_n_total"]) == n
        assert r["uneven_calls"].tolist() == [2, 8] + [P.param_count(S, A)] * 11 + [2]
    for k in GLOBALS:  # rank against rank: every global entry bit for bit
        assert same(ranks[0][f"uneven_{k}"], ranks[1][f"uneven_{k}"]), k
    one = union_update(n, whiten=True)
    ref_theta, ref_npg, ref_kl, ref_adv = restated_update(n)
    # the ranks' own rows, whitened with the global statistics (fp64: a few ulps of the restatement)
    got_adv = np.concatenate([ranks[0]["uneven_adv"], ranks[1]["uneven_adv"]])
    assert got_adv.shape == (n,) and np.abs(got_adv - ref_adv).max() <= 1e-12 * np.abs(ref_adv).max()

    def errors(theta, npg, kl):
        return (np.linalg.norm(theta.astype(np.float64) - ref_theta), np.linalg.norm(npg - ref_npg), abs(kl - ref_kl))
    dp = errors(ranks[0]["uneven_theta"], ranks[0]["uneven_npg"], ranks[0]["uneven_scal"][3])
    sp = errors(one["theta"], one["npg"], one["scal"][3])
    print("DP_ERR theta %.3e | %.3e  npg_grad %.3e | %.3e (|npg| %.3e)  kl_dist %.3e | %.3e (kl %.3e)" %
          (dp[0], sp[0], dp[1], sp[1], np.linalg.norm(ref_npg), dp[2], sp[2], ref_kl))
    for name, e_dp, e_sp in zip(("theta", "npg_grad", "kl_dist"), dp, sp):
        assert e_dp <= 2.0 * e_sp, (name, e_dp, e_sp)
