"""The f16x3 ensemble forward at the lane counts that reach each 16x16x32 tile, as named tensors.

`runs()` builds one (197, 36) ensemble of 4 x [512] * 4 from a numpy.random.RandomState seed and
runs one forward per case: 8192 lanes (256 x 256 hidden, 128 x 224 output tiles), 5120 (the 160-row
block tiles, 80 x 224 output), 4096 (128-row block tiles, stream-K output), 512 (128 x 64 / 128 x 32
small-row tiles, stream-K over K), 128 and 512 member-blocked (128 rows per member: the small-row
tiles at 8 waves).  Per case it returns the predictions, the activation buffer (x0 and every hidden
slice) and every row-exponent slot.

The weights and rows are chosen for the launch prologue and epilogue, which handle the row
exponents: member 3's second hidden layer has zero weights and bias -1 (an all-zero slice: its
slot holds the clamp, -100); the last hidden layer's weights are 8 x larger (rows whose maximum
lies in the last slice); rows 0-7 sit exactly at the normalizer mean (x0 = 0: slot 0 at the
clamp), row 8 carries an inf, row 9 a NaN, rows 16-23 lie 1e4 x and rows 24-31 1e-4 x the offline
scale from the mean.  `row_classes()` counts them from the recorded slots.

test_gpu_h3_bits.py compares the SHA-256 of every tensor's bytes with tests/golden/g19_h3_bits.json,
which `python tests/h3_bits.py --record PATH` writes (per tensor the digest and, for diagnosis,
its fp64 sum over finite values).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

DEV = "cuda"
S, A, H, L, M = 197, 36, 512, 4, 4
# (name, lanes, member-blocked)
CASES = (("8192", 8192, False), ("5120", 5120, False), ("4096", 4096, False), ("512", 512, False),
         ("128", 128, False), ("b512", 512, True))


def _weights(rs):
    ws = []
    for m in range(M):
        layers = []
        for i in range(L + 1):
            in_dim, out_dim = S + A + i * H, (S if i == L else H)
            k = 1.0 / np.sqrt(in_dim)
            W = rs.uniform(-k, k, (out_dim, in_dim)).astype(np.float32)
            b = rs.uniform(-k, k, out_dim).astype(np.float32)
            if i == L - 1:
                W, b = W * 8.0, b * 8.0
            if m == 3 and i == 1:
                W, b = np.zeros_like(W), np.full_like(b, -1.0)
            layers.append((torch.from_numpy(W), torch.from_numpy(b)))
        ws.append(layers)
    return ws


def _rows(rs, B, mu_s, mu_a):
    ob = mu_s + 0.5 * rs.randn(B, S)
    ac = mu_a + rs.randn(B, A)
    ob[:8], ac[:8] = mu_s, mu_a
    ob[8, 3] = np.inf
    ob[9, 5] = np.nan
    ob[16:24] = mu_s + (ob[16:24] - mu_s) * 1e4
    ac[16:24] = mu_a + (ac[16:24] - mu_a) * 1e4
    ob[24:32] = mu_s + (ob[24:32] - mu_s) * 1e-4
    ac[24:32] = mu_a + (ac[24:32] - mu_a) * 1e-4
    return ob, ac


def runs():
    """{case.tensor: numpy array}"""
    if os.path.dirname(os.path.dirname(os.path.abspath(__file__))) not in sys.path:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import amp_extensions_amd as amx
    rs = np.random.RandomState(1901)
    # normalizers exactly representable in fp32 (rows at the mean give x0 = 0 exactly)
    mu_s = rs.randn(S).astype(np.float32).astype(np.float64)
    mu_a = rs.randn(A).astype(np.float32).astype(np.float64)
    norms = [torch.from_numpy(x.astype(np.float32)) for x in
             (mu_s, rs.uniform(0.5, 2.0, S), mu_a, rs.uniform(0.5, 2.0, A), 0.01 * rs.randn(S),
              rs.uniform(0.005, 0.02, S))]
    ctx = amx.AmxContext(S, A, n_models=M, hidden=H, n_hidden=L, feat_dim=512, device=DEV)
    ens = amx.DeviceEnsemble(ctx, _weights(rs), norms)
    out = {}
    for name, B, blocked in CASES:
        ob, ac = _rows(np.random.RandomState(B + blocked), B, mu_s, mu_a)
        obd, acd = torch.from_numpy(ob).to(DEV), torch.from_numpy(ac).to(DEV)
        if blocked:
            preds = ens.forward_blocked(obd, acd, B // M)
            ws = ens.workspace_blocked(B // M)
        else:
            preds = ens.forward_preds(obd, acd, B)
            ws = ens.workspace(B)
        torch.cuda.synchronize()
        out[f"{name}.preds"] = preds.cpu().numpy()
        out[f"{name}.act"] = ws["act"].cpu().numpy()
        out[f"{name}.rexp"] = ws["rexp"].cpu().numpy()
    return out


def row_classes(rexp):
    """Counts over a case's slots [M][L + 1][rows]: slots at the clamps and rows (of any member)
    whose largest exponent is the last slice's alone."""
    last_max = (rexp[:, L] > rexp[:, :L].max(axis=1)).sum()
    return dict(clamp_lo=int((rexp == -100).sum()), clamp_hi=int((rexp == 100).sum()), last_max=int(last_max))


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def finite_sum(x):
    x = x.astype(np.float64)
    return float(np.where(np.isfinite(x), x, 0.0).sum())


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: h3_bits.py --record PATH")
    t = runs()
    rec = {n: dict(sha256=digest(x), finite_sum=finite_sum(x)) for n, x in sorted(t.items())}
    for name, _, _ in CASES:
        rec[f"{name}.rexp"]["classes"] = row_classes(t[f"{name}.rexp"])
        print(name, rec[f"{name}.rexp"]["classes"], rec[f"{name}.preds"]["sha256"][:16], flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
