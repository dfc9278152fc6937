"""Time the MLP-feature MMD cost (MLPCost) at run.py's shape -- S/A 197/36, hidden_dims [512] * 4,
F 512, 40 960 rollout rows (8192 lanes x 5 steps), 50 000 expert rows -- and write
profiles/mlpcost_time.txt:
  * us per MlpMap.features pass over the rollout's rows and per layer (HIP events around REPS
    back-to-back launches, after a warm-up);
  * rollout + relabel of the same engine with an MLPCost and with an RBFLinearCost, in the same
    run, eager and as a replayed HIP graph;
  * the torch-CPU fit_cost + get_costs of the same net on the same rows (what the reference's
    MLPCost runs per rollout), on 16 threads.
Reported, not gated.  usage: python tools/mlpcost_time.py"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import amp_extensions_amd as amx  # noqa: E402
from amp_extensions_amd import _native as N  # noqa: E402
from amp_extensions_amd import synthetic as syn  # noqa: E402
from amp_extensions_amd.ensemble import init_ensemble_weights  # noqa: E402
from amp_extensions_amd.policy import init_mlp_policy_params  # noqa: E402

S, A, F, B, K, NE = 197, 36, 512, 8192, 5, 50000
HIDDEN = [512] * 4
REPS = 20
DEV = "cuda"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    s, a, s2 = syn.offline(2048, S, A, 0)
    t32 = lambda x: torch.as_tensor(x).float()
    from amp_extensions_amd.datasets import get_transformations
    norms = get_transformations(t32(s), t32(a), t32(s2))
    ctx = amx.AmxContext(S, A, n_models=4, hidden=512, n_hidden=4, feat_dim=F, device=DEV)
    ens = amx.DeviceEnsemble(ctx, init_ensemble_weights(S, A, HIDDEN, 4, 100), norms)
    ens.compute_threshold(t32(s).to(DEV), t32(a).to(DEV))
    expert = t32(syn.expert(NE, S, 3))
    mlp = amx.MLPCost(expert, hidden_dims=HIDDEN, feature_dim=F, lambda_b=0.0025, seed=100, ctx=ctx)
    rbf = amx.RBFLinearCost(expert, feature_dim=F, lambda_b=0.0025, seed=100, ctx=ctx)
    say(f"MLPCost at run.py's shape: S/A {S}/{A}, hidden_dims {HIDDEN}, F {F}, {B * K} rollout rows ({B} lanes x {K} "
        f"steps), {NE} expert rows; device {torch.cuda.get_device_name(0)}, {ctx.n_cus} CUs; {REPS} launches per figure")

    # ---- the features pass and its layers --------------------------------------------------
    rows, m = B * K, mlp.map
    x = torch.zeros(rows, m.Kp, device=DEV)
    x[:, :m.D] = t32(syn.expert(rows, S, 4)).to(DEV)
    phi = torch.empty(rows, F, device=DEV)
    part = torch.empty(rows // N.RFF_PART_ROWS, F, dtype=torch.float64, device=DEV)
    us_mlp = timed(lambda: m.features(x, rows, rows, phi, part))
    us_rff = timed(lambda: rbf.map.features(x, rows, rows, phi, part))
    flops = 2 * rows * sum(L[3] * L[4] for L in m.layers)
    say(f"MlpMap.features ({rows} rows, row exponents computed): {us_mlp:8.1f} us  ({flops / us_mlp / 1e6:.0f} TFLOP/s "
        f"algorithmic); RffMap.features on the same rows: {us_rff:.1f} us")
    bufs, rexp = m._workspace(rows)
    lib, h = ctx.lib, ctx.h
    src, ld, re_in = x, m.Kp, rexp[0]
    for i, (W2, wexp, b, out_p, k_pad) in enumerate(m.layers[:-1]):
        o = bufs[i & 1]

        def layer(src=src, ld=ld, re_in=re_in, o=o, W2=W2, wexp=wexp, b=b, out_p=out_p, k_pad=k_pad, i=i):
            N.check(lib.amx_gemm_bias_act_h3(h, 1, rows, out_p, k_pad, src.data_ptr(), ld, 0, W2.data_ptr(), 0,
                                             wexp.data_ptr(), 0, b.data_ptr(), 0, o.data_ptr(), out_p, 0, 0,
                                             N.AMX_ACT_RELU, re_in.data_ptr(), 0, 1, rexp[i + 1].data_ptr(), 0,
                                             ctx.stream), "hidden")
        us = timed(layer)
        say(f"  hidden layer {i} (K {k_pad:3d} -> {out_p}, ReLU, amx_gemm_bias_act_h3): {us:7.1f} us  "
            f"({2 * rows * out_p * k_pad / us / 1e6:.0f} TFLOP/s)")
        src, ld, re_in = o, out_p, rexp[i + 1]
    W2, wexp, b, _, k_pad = m.layers[-1]

    def last():
        N.check(lib.amx_mlp_features_h3(h, rows, rows, F, k_pad, src.data_ptr(), ld, W2.data_ptr(), wexp.data_ptr(),
                                        re_in.data_ptr(), b.data_ptr(), m.scale, phi.data_ptr(), F, part.data_ptr(),
                                        None, ctx.stream), "features")
    us = timed(last)
    say(f"  feature layer (K {k_pad} -> {F}, cos(tanh(.)) in fp64, phi rows + fp64 column partials, "
        f"amx_mlp_features_h3): {us:7.1f} us  ({2 * rows * F * k_pad / us / 1e6:.0f} TFLOP/s)")

    # ---- rollout + relabel, MLPCost beside RBFLinearCost -----------------------------------
    pw, ls = init_mlp_policy_params(S, A)
    table = syn.reset_table(65536, S, 1)
    for name, cost in (("RBFLinearCost", rbf), ("MLPCost", mlp)):
        pol = amx.DevicePolicy(ctx, pw, ls, seed=1000)
        eng = amx.RolloutEngine(ens, table, lanes=B, policy=pol, cost=cost, seed=7, max_steps=K)
        eng.reset_all()

        def eager(eng=eng, cost=cost):
            eng.rollout()
            eng.relabel()
            cost.get_expert_cost()
        us_e = timed(eager, reps=10)
        replay = eng.graph_rollout(K, tail=cost.get_expert_cost)
        us_g = timed(replay, reps=10)
        say(f"rollout + relabel + expert cost, {name:13s}: eager {us_e / 1e3:7.3f} ms, graph replay {us_g / 1e3:7.3f} ms "
            f"per {B * K} transitions")

    # ---- what it replaces: the torch-CPU fit_cost + get_costs of the same net ---------------
    n_thr = torch.get_num_threads()
    torch.set_num_threads(16)
    xc = x[:, :m.D].cpu()
    net, scale = mlp.net, np.sqrt(2 / F)
    with torch.no_grad():
        phi_e = (torch.cos(net(expert[:1024])) * scale).mean(0)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            w = (torch.cos(net(xc)) * scale).mean(0) - phi_e                                    # fit_cost
            torch.clamp(torch.mm(torch.cos(net(xc)) * scale, w.unsqueeze(1)), -1.0, 0.0)       # get_costs
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    torch.set_num_threads(n_thr)
    say(f"torch-CPU ({torch.__version__}, 16 threads) fit_cost + get_costs of the same net on the same {rows} rows "
        f"(two passes of the net, as the reference): {best * 1e3:.0f} ms  (x{best * 1e6 / us_mlp:.0f} the device's "
        f"one features pass)")
    out = os.path.join(ROOT, "profiles", "mlpcost_time.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
