"""The device fits and the 64 x 64 f32 products at their smallest shapes, as named tensors.

`runs()` trains the value baseline (amx_vfit_epoch), the dynamics ensemble (amx_efit_step), the
discriminator (amx_dfit_step) and the behaviour-cloning policy (amx_bcfit_steps) and calls the
three product entry points once each; every input comes from a numpy.random.RandomState seed.
test_gpu_fit_bits.py compares the SHA-256 of every tensor's bytes with tests/golden/g18_fit_bits.npz,
which `python tests/fit_bits.py --record PATH` writes: per tensor the digest and, for diagnosis,
the fp64 sum, max |x| and the first 16 values; torch.version.hip and hipcc's version line as text.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import torch

DEV = "cuda"


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV).contiguous()


def _host(t):
    return t.detach().cpu().contiguous().numpy()


def _linear(rs, out_dim, in_dim):
    """nn.Linear-sized uniform weights from a RandomState."""
    k = 1.0 / np.sqrt(in_dim)
    return (rs.uniform(-k, k, (out_dim, in_dim)).astype(np.float32), rs.uniform(-k, k, out_dim).astype(np.float32))


# ---- value baseline ------------------------------------------------------------------------------

def run_vfit(out):
    """(226, 28) context, hidden (128, 128), 333 rows in paths of 50, 100, 3 and 180: one epoch of
    4 steps, lr 1e-3, reg 1e-3."""
    import amp_extensions_amd as amx
    S, hidden, lens = 226, (128, 128), (50, 100, 3, 180)
    ctx = amx.AmxContext(S, 28, n_models=4, hidden=64, n_hidden=4, feat_dim=128, device=DEV)
    rs = np.random.RandomState(1801)
    sizes = [S + 4, *hidden, 1]
    layers = [_linear(rs, sizes[i + 1], sizes[i]) for i in range(3)]
    paths = []
    for l in lens:
        obs = rs.randn(l, S) * 4.0
        obs[:, 3] *= 6.0
        paths.append(dict(observations=obs, rewards=np.zeros(l, dtype=np.float32), returns=rs.randn(l) * 2.0 + 1.0))
    perm = rs.permutation(sum(lens))
    bl = amx.DeviceMLPBaseline(ctx, layers, learn_rate=1e-3, reg_coef=1e-3, epochs=1)
    _, _, losses = bl.fit(paths, return_errors=True, return_all_errors=True, perms=[perm])
    torch.cuda.synchronize()
    for name, t in zip(("W0", "b0", "W1", "b1", "w2", "b2"), (bl.W[0], bl.b[0], bl.W[1], bl.b[1], bl.w_head, bl.b_head)):
        out[f"vfit.{name}"] = _host(t)
    m, v, step = bl._adam
    out["vfit.exp_avg"], out["vfit.exp_avg_sq"], out["vfit.step"] = _host(m), _host(v), _host(step)
    out["vfit.epoch_loss"] = np.concatenate(losses).astype(np.float32)


# ---- dynamics ensemble ---------------------------------------------------------------------------

def _transitions(rs, n, S, A, power):
    s = 0.5 * rs.randn(n, S) ** power
    a = rs.randn(n, A) ** power
    Q = rs.randn(S + A, S) / np.sqrt(S + A)
    s2 = s + 0.05 * np.tanh(np.concatenate([s, a], 1) @ Q) + 0.01 * rs.randn(n, S)
    return tuple(torch.from_numpy(x).float() for x in (s, a, s2))


def _batches(rs, n, batch, M):
    """(idx [M][steps][batch], sizes) of one shuffled pass of every member over n rows."""
    steps = -(-n // batch)
    idx = np.zeros((M, steps, batch), dtype=np.int32)
    for g in range(M):
        p = rs.permutation(n)
        for s in range(steps):
            rows = p[s * batch:(s + 1) * batch]
            idx[g, s, :len(rows)] = rows
    return idx, [min(batch, n - s * batch) for s in range(steps)]


def run_efit(out, name, seed, n, nv, batch, optim, lr, p1, clip, epochs, power):
    """test_gpu_efit.py's case `name` at engine level: S, A = 24, 6, hidden [32, 32], 4 members."""
    from amp_extensions_amd.engine import AmxContext, DeviceEnsemble
    S, A, hidden, M = 24, 6, 32, 4
    rs = np.random.RandomState(seed)
    tr = _transitions(rs, n, S, A, power)
    va = _transitions(rs, nv, S, A, power) if nv else None
    weights = [[_linear(rs, hidden if i < 2 else S, S + A + i * hidden) for i in range(3)] for _ in range(M)]
    d = tr[2] - tr[0]
    norms = (tr[0].mean(0), tr[0].std(0), tr[1].mean(0), tr[1].std(0), d.mean(0), d.std(0))
    ctx = AmxContext(S, A, n_models=M, hidden=hidden, n_hidden=2, device=DEV)
    eng = DeviceEnsemble(ctx, weights, norms, gemm="f32")
    eng.fit_begin(tr, optim, lr, p1, batch, val_data=va)
    losses = []
    for _ in range(epochs):
        idx, sizes = _batches(rs, n, batch, M)
        losses.append(eng.fit_epoch(idx, sizes, train=True, grad_clip=clip))
        if nv:
            idx, sizes = _batches(rs, nv, batch, M)
            losses.append(eng.fit_epoch(idx, sizes, train=False, split="val"))
    torch.cuda.synchronize()
    f = eng._fit
    for i in range(3):
        out[f"efit.{name}.W{i}"], out[f"efit.{name}.b{i}"] = _host(eng.W[i]), _host(eng.b[i])
    out[f"efit.{name}.state1"], out[f"efit.{name}.step"] = _host(f["s1"]), _host(f["step"])
    if f["s2"] is not None:
        out[f"efit.{name}.state2"] = _host(f["s2"])
    out[f"efit.{name}.losses"] = np.concatenate(losses, axis=1).astype(np.float32)
    eng.fit_end()


# ---- discriminator ------------------------------------------------------------------------------

def _rows(rs, n, S, scale, shift):
    s = scale * rs.randn(n, S) + shift
    return np.concatenate([s, s + 0.1 * rs.randn(n, S)], 1).astype(np.float32)


def run_dfit(out, ctx, loss, optim):
    """test_gpu_dfit.py's small shape: D 48, hidden [64, 32], bs 37, grad_lambda 10, reg_coef 0.05,
    scaling_coef 0.5, three steps at lr 1e-3."""
    from amp_extensions_amd import _native as N
    S, h0, h1, bs, steps = 24, 64, 32, 37, 3
    D, Dp, H0p, H1p, Bt = 2 * S, 64, 128, 128, 64
    rs = np.random.RandomState(1816)
    expert = _dev(_rows(rs, 90, S, 0.5, 0.3))
    W0, b0 = _linear(rs, h0, D)
    W1, b1 = _linear(rs, h1, h0)
    w2, b2 = _linear(rs, 1, h1)
    pad = lambda x, shape: np.pad(x, [(0, p - s) for s, p in zip(x.shape, shape)])  # noqa: E731
    t = [_dev(pad(W0, (H0p, Dp))), _dev(pad(b0, (H0p,))), _dev(pad(W1, (H1p, H0p))), _dev(pad(b1, (H1p,))),
         _dev(pad(w2[0], (H1p,))), _dev(pad(b2, (4,)))]
    lib = ctx.lib
    P = lib.amx_dfit_param_count(Dp, H0p, H1p)
    s1 = torch.zeros(P, device=DEV)
    s2 = torch.zeros(P, device=DEV) if optim == "adam" else None
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    work = torch.zeros(lib.amx_dfit_work_floats(Dp, H0p, H1p, Bt), device=DEV)
    metrics = torch.zeros(steps, 8, dtype=torch.float64, device=DEV)
    for k in range(steps):
        idx = _dev(rs.randint(0, 90, bs), torch.int32)
        agent = _dev(_rows(rs, bs, S, 0.7, -0.2))
        N.check(lib.amx_dfit_step(ctx.h, N.AMX_DISC_LEAST_SQUARES if loss == "ls" else N.AMX_DISC_LOG_LIKELIHOOD,
                                  N.AMX_DFIT_ADAM if optim == "adam" else N.AMX_DFIT_SGD, 1e-3,
                                  1e-8 if optim == "adam" else 0.9, 0.5, 0.05, 10.0, bs, Bt, D, Dp, H0p, H1p,
                                  idx.data_ptr(), None, expert.data_ptr(), expert.stride(0), 90, agent.data_ptr(),
                                  agent.stride(0), bs, *[x.data_ptr() for x in t], s1.data_ptr(), N.ptr(s2),
                                  step.data_ptr(), work.data_ptr(), metrics[k].data_ptr(), ctx.stream), "amx_dfit_step")
        torch.cuda.synchronize()
    tag = f"dfit.{loss}_{optim}"
    for name, x in zip(("W0", "b0", "W1", "b1", "w2", "b2"), t):
        out[f"{tag}.{name}"] = _host(x)
    out[f"{tag}.state1"], out[f"{tag}.step"], out[f"{tag}.metrics"] = _host(s1), _host(step), _host(metrics)
    if s2 is not None:
        out[f"{tag}.state2"] = _host(s2)


# ---- behaviour cloning -----------------------------------------------------------------------------

def run_bcfit(out, ctx, loss_type):
    """test_gpu_bcfit.py's ragged inputs (S / A = 197 / 36, paths of 70, 130, 3 and 120 rows): ten
    steps cut into two launches."""
    import amp_extensions_amd as amx
    S, A, lens = 197, 36, (70, 130, 3, 120)
    rs = np.random.RandomState(1817)
    Wt = rs.randn(S, A) * 0.05
    obs = np.concatenate([rs.randn(l, S) for l in lens])
    act = np.tanh(obs @ Wt) + 0.1 * rs.randn(len(obs), A)
    theta = np.concatenate([np.concatenate([w.ravel(), b]) for w, b in
                            (_linear(rs, 32, S), _linear(rs, 32, 32), _linear(rs, A, 32))] + [np.full(A, -0.25)])
    batches = rs.choice(len(obs), size=(2, 5, 64))
    dbc = amx.DeviceBC(ctx, theta.astype(np.float32), loss_type=loss_type)
    dbc.fit(obs, act, 2, batches=batches, max_steps_per_launch=5)
    torch.cuda.synchronize()
    m, v, step = dbc._adam_state()
    tag = f"bcfit.{loss_type}"
    out[f"{tag}.theta"], out[f"{tag}.exp_avg"], out[f"{tag}.exp_avg_sq"] = _host(dbc.theta), _host(m), _host(v)
    out[f"{tag}.step"], out[f"{tag}.step_losses"] = _host(step), np.asarray(dbc.step_losses, dtype=np.float32)


# ---- the three products ----------------------------------------------------------------------------

def run_gemms(out, ctx):
    from amp_extensions_amd import _native as N
    lib, rs = ctx.lib, np.random.RandomState(1818)
    rn = lambda *shape: _dev(rs.randn(*shape))  # noqa: E731
    # amx_gemm_bias_act_t64: 2 groups, 128 rows, N 64, K 96, ReLU, in place at col_off = K
    G, rows, Nn, K = 2, 128, 64, 96
    A, W, b = rn(G, rows, K + Nn), rn(G, Nn, K), rn(G, Nn)
    N.check(lib.amx_gemm_bias_act_t64(ctx.h, G, rows, Nn, K, A.data_ptr(), K + Nn, rows * (K + Nn), W.data_ptr(), K,
                                      Nn * K, b.data_ptr(), Nn, A.data_ptr(), K + Nn, rows * (K + Nn), K,
                                      N.AMX_ACT_RELU, ctx.stream), "amx_gemm_bias_act_t64")
    out["gemm.t64"] = _host(A)
    # amx_gemm_nn_f32: M 128, N 68, K 64, mask rows wrap at 64
    M, Nn, K, ld = 128, 68, 64, 72
    A, B, mask = rn(M, K), rn(K, ld), rn(64, ld)
    C = torch.zeros(M, ld, device=DEV)
    N.check(lib.amx_gemm_nn_f32(ctx.h, M, Nn, K, A.data_ptr(), K, B.data_ptr(), ld, C.data_ptr(), ld, mask.data_ptr(),
                                ld, 64, ctx.stream), "amx_gemm_nn_f32")
    out["gemm.nn"] = _host(C)
    # amx_gemm_tn_f32: R 96, M 64, N 68, mask, column sums over 70 of the 96 rows
    R, M = 96, 64
    A, B, mask = rn(R, M), rn(R, ld), rn(M, ld)
    C, cs = torch.zeros(M, ld, device=DEV), torch.zeros(M, device=DEV)
    N.check(lib.amx_gemm_tn_f32(ctx.h, R, M, Nn, A.data_ptr(), M, B.data_ptr(), ld, C.data_ptr(), ld, mask.data_ptr(),
                                ld, cs.data_ptr(), 70, ctx.stream), "amx_gemm_tn_f32")
    torch.cuda.synchronize()
    out["gemm.tn"], out["gemm.tn_colsum"] = _host(C), _host(cs)


def runs():
    """name -> numpy array of every pinned tensor."""
    from amp_extensions_amd.engine import AmxContext
    out = {}
    run_vfit(out)
    adam = dict(optim="adam", lr=1e-3, p1=1e-8)
    sgd = dict(optim="sgd", lr=0.1, p1=0.9)
    run_efit(out, "a_adam_clip", 1811, n=600, nv=300, batch=256, clip=1.0, epochs=2, power=3, **adam)
    run_efit(out, "c_ragged", 1813, n=250, nv=0, batch=100, clip=0.25, epochs=1, power=1, **sgd)
    small = AmxContext(4, 1, n_models=1, hidden=128, n_hidden=0, feat_dim=128, device=DEV)
    for loss in ("ls", "ll"):
        for optim in ("sgd", "adam"):
            run_dfit(out, small, loss, optim)
    bc_ctx = AmxContext(197, 36, n_models=1, hidden=16, n_hidden=1, feat_dim=256, device=DEV)
    for loss_type in ("MSE", "MLE"):
        run_bcfit(out, bc_ctx, loss_type)
    run_gemms(out, small)
    return out


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def summary(x):
    """(fp64 sum, max |x|, first 16 values) of a tensor, for diagnosis."""
    v = np.asarray(x, dtype=np.float64).ravel()
    head = np.zeros(16)
    head[:min(16, v.size)] = v[:16]
    return float(v.sum()), float(np.abs(v).max()) if v.size else 0.0, head


def record(path):
    from amp_extensions_amd import _build
    out = runs()
    names = sorted(out)
    sums = [summary(out[n]) for n in names]
    ver = subprocess.run([_build._hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines()
    np.savez_compressed(path, names=np.array(names), sha256=np.array([digest(out[n]) for n in names]),
             sum=np.array([s[0] for s in sums]), maxabs=np.array([s[1] for s in sums]),
             head=np.stack([s[2] for s in sums]), torch_hip=np.array(str(torch.version.hip)),
             hipcc=np.array(next((l for l in ver if "HIP version" in l), ver[0] if ver else "")))
    print(f"recorded {len(names)} tensors to {path}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: fit_bits.py --record PATH")
    record(sys.argv[2])
