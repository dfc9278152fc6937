"""Hash of the ensemble forward (every lane-count regime of the f16x3 tiles: 256x256, row-block,
stream-K and small-tile shapes, at S = 197 and S = 226; one large and one small forward of the
bf16x6 and f32 paths), of the RFF passes (every f16x3 RFF tile, one pass of the other two
paths) and of the f16x3 launches at a K that is a multiple of 16 but not of 32 (raw C calls:
no Python surface pads K to less than 32), for bit-identity checks between library builds
(tools/so_ab.sh).  usage: python tools/fwd_hash.py"""
import hashlib
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import amp_extensions_amd as amx  # noqa: E402
from amp_extensions_amd import _native as N  # noqa: E402
from amp_extensions_amd import synthetic as syn  # noqa: E402
from amp_extensions_amd.datasets import get_transformations  # noqa: E402
from amp_extensions_amd.engine import split_f16x2  # noqa: E402
from amp_extensions_amd.ensemble import init_ensemble_weights  # noqa: E402

h = hashlib.sha256()


def ensemble(S, A, gemms):
    s, a, s2 = syn.offline(20000, S, A, 0)
    norms = get_transformations(*(torch.from_numpy(x).float() for x in (s, a, s2)))
    ctx = amx.AmxContext(S, A, n_models=4, hidden=512, n_hidden=4, feat_dim=512, device="cuda")
    w = init_ensemble_weights(S, A, [512] * 4, 4, base_seed=100)
    return ctx, {g: amx.DeviceEnsemble(ctx, w, norms, gemm=g) for g in gemms}


def forwards(tag, ens, S, A, lanes):
    for B in lanes:
        rs = np.random.RandomState(B)
        ob = torch.from_numpy(0.5 * rs.randn(B, S)).cuda()
        ac = torch.from_numpy(rs.randn(B, A)).cuda()
        p = ens.forward_preds(ob, ac, B)[:, :B].contiguous()
        h.update(p.cpu().numpy().tobytes())
        print(f"{tag} lanes {B}: preds sum {p.double().sum().item():.17g}", flush=True)


def rff_passes(tag, rff, D, g, row_counts):
    for rows in row_counts:
        x = torch.zeros(rows, rff.Kp, device="cuda")
        x[:, :D] = 0.5 * torch.randn(rows, D, generator=g).cuda()
        phi = torch.empty(rows, 512, device="cuda")
        part = torch.empty((rows + 127) // 128 * 4, 512, dtype=torch.float64, device="cuda")  # 32-row partials
        rff.features(x, rows, rows, phi, part)
        torch.cuda.synchronize()
        h.update(phi.cpu().numpy().tobytes())
        h.update(part.cpu().numpy().tobytes())
        print(f"{tag} rff {rows}: phi sum {phi.double().sum().item():.17g}", flush=True)


def k48(ctx):
    """K = 48 (the BK-16 tiles: 128 x 128 hidden / RFF, 128 x 224 output) through the C ABI."""
    lib, s, K, rows = ctx.lib, ctx.stream, 48, 256
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(rows, K, generator=g) * torch.exp(4 * torch.randn(rows, 1, generator=g))).cuda()
    rexp = torch.empty(rows, dtype=torch.int32, device="cuda")
    N.check(lib.amx_row_exponents(ctx.h, 1, rows, K, x.data_ptr(), K, 0, rexp.data_ptr(), rows, 1, s), "row_exp")
    W2h, weh = split_f16x2(ctx, (torch.randn(1, 128, K, generator=g) / 3.0).cuda())
    W2o, weo = split_f16x2(ctx, (torch.randn(1, 256, K, generator=g) / 3.0).cuda())
    W2r, wer = split_f16x2(ctx, (torch.randn(1, 512, K, generator=g) / 3.0).cuda())
    bias = torch.randn(512, generator=g).cuda()
    hid = torch.zeros(rows, 128, device="cuda")
    rout = torch.full((rows,), -100, dtype=torch.int32, device="cuda")
    N.check(lib.amx_gemm_bias_act_h3(ctx.h, 1, rows, 128, K, x.data_ptr(), K, 0, W2h.data_ptr(), 128 * 2 * K,
                                     weh.data_ptr(), 128, bias.data_ptr(), 0, hid.data_ptr(), 128, 0, 0,
                                     N.AMX_ACT_RELU, rexp.data_ptr(), rows, 1, rout.data_ptr(), 0, s), "bias_act_h3")
    preds = torch.zeros(rows, ctx.S, device="cuda")
    N.check(lib.amx_gemm_out_unnorm_h3(ctx.h, 1, rows, ctx.S, K, x.data_ptr(), K, 0, W2o.data_ptr(), 256 * 2 * K,
                                       weo.data_ptr(), 256, bias.data_ptr(), 0, preds.data_ptr(), ctx.S, 0,
                                       rexp.data_ptr(), rows, 1, 0, s), "out_unnorm_h3")
    phi = torch.empty(rows, 512, device="cuda")
    part = torch.empty(rows // 32, 512, dtype=torch.float64, device="cuda")
    N.check(lib.amx_rff_features_h3(ctx.h, rows, rows - 5, 512, K, x.data_ptr(), K, W2r.data_ptr(), wer.data_ptr(),
                                    rexp.data_ptr(), bias.data_ptr(), 0.0625, phi.data_ptr(), 512, part.data_ptr(),
                                    None, s), "rff_features_h3")
    torch.cuda.synchronize()
    for t in (hid, rout, preds, phi, part):
        h.update(t.cpu().numpy().tobytes())
    print(f"K 48: hidden sum {hid.double().sum().item():.17g} preds sum {preds.double().sum().item():.17g} "
          f"phi sum {phi.double().sum().item():.17g}", flush=True)


S, A = 197, 36
ctx, ens = ensemble(S, A, ("f16x3", "bf16x6", "f32"))
forwards("f16x3", ens["f16x3"], S, A, (8192, 7168, 6144, 5120, 4096, 2048, 1000, 640, 128))
for gm in ("bf16x6", "f32"):
    forwards(gm, ens[gm], S, A, (8192, 640))
ctx226, ens226 = ensemble(226, 28, ("f16x3",))
forwards("S226 f16x3", ens226["f16x3"], 226, 28, (5120, 2048))
g = torch.Generator().manual_seed(3)
W = torch.randn(512, 2 * S, generator=g) / 3.0
b = torch.rand(512, generator=g) * 6.28
rff_passes("f16x3", amx.RffMap(ctx, W, b), 2 * S, g, (40960, 21504, 12288, 5120))
for gm in ("bf16x6", "f32"):
    rff_passes(gm, amx.RffMap(ctx, W, b, gemm=gm), 2 * S, g, (5120,))
k48(ctx)
print("HASH", h.hexdigest(), flush=True)
