"""Time the NPG update with a subsampled Fisher and a BC term (DeviceNPG with hvp_sample_frac < 1,
bc=...) at the rollout shape 40 960 x 197 / 36, and write profiles/npgreg_time.txt:

  * one Fisher-vector pass over an index vector (amx_npg_pass_idx, theta cache on) against the
    obvious alternative: index_select of the rows (and of their cached forward) into scratch
    buffers, then the plain pass;
  * the whole update at frac 1, 0.5 and 0.25, with and without a 4 096-row BC set, against the
    frac = 1 update of another tree (--parent PATH: a checkout of the parent commit with its
    library built), in alternating child processes on the same box;
  * the restated fp32 torch loop (tests/npgreg_ref.py) on the host's threads.

usage: python tools/npgreg_time.py [--parent PATH] [--threads 16] [--out profiles/npgreg_time.txt]
       python tools/npgreg_time.py --update-only FRAC BC   (the child: prints one update time)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, A, NE, REG = 40960, 197, 36, 4096, 0.1


def inputs():
    rs = np.random.RandomState(0)
    obs = (0.5 * rs.randn(N, S)).astype(np.float32)
    act = rs.randn(N, A).astype(np.float32)
    adv = rs.randn(N)
    eo, ea = (0.5 * rs.randn(NE, S)).astype(np.float32), rs.randn(NE, A).astype(np.float32)
    return obs, act, adv, eo, ea


def device_npg(root, frac):
    sys.path.insert(0, root)
    import amp_extensions_amd as amx
    from amp_extensions_amd.policy import init_mlp_policy_params
    layers, ls = init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25)
    ctx = amx.AmxContext(S, A, n_models=1, hidden=128, n_hidden=1, device="cuda")
    kw = {} if frac >= 0.99 else {"hvp_sample_frac": frac}
    return amx.DeviceNPG(ctx, layers, ls, normalized_step_size=0.1, min_log_std=-2.0, **kw)


def update_ms(root, frac, bc, reps=20):
    """Consecutive updates (the training loop's form), the one host sync of each included."""
    npg = device_npg(root, frac)
    obs, act, adv, eo, ea = (torch.from_numpy(x).cuda() for x in inputs())
    kw = {"bc": (eo, ea, REG)} if bc else {}
    np.random.seed(0)
    for _ in range(3):
        npg.train_from_arrays(obs, act, adv, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        npg.train_from_arrays(obs, act, adv, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def child(root, frac, bc):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--update-only", str(frac), str(int(bc)), "--root",
                          root], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return float(out.stdout.strip().split()[-1])


def pass_times(lines):
    from amp_extensions_amd.npg import NPG_FVP, NPG_VPG
    npg = device_npg(ROOT, 1.0)
    obs, act, adv, _, _ = (torch.from_numpy(x).cuda() for x in inputs())
    o, a, ad = npg._inputs(obs, act, adv)
    hc = npg._hcache(N)
    npg._pass(NPG_VPG, o, a, ad, None, hcache=hc)
    vec = torch.randn(npg.P, device="cuda")

    def timed(fn, reps=50):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    lines.append(f"one Fisher-vector pass (theta cache on, partials only), us per pass, {N} x {S} / {A}:")
    lines.append(f"  all {N} rows, plain pass: {timed(lambda: npg._pass(NPG_FVP, o, a, None, vec, hcache=hc, reduce=False)):.1f}")
    for frac in (0.5, 0.25):
        m = int(frac * N)
        idx = torch.from_numpy(np.random.RandomState(1).choice(N, size=m).astype(np.int32)).cuda()
        li = idx.long()
        so, sh = torch.empty(m, S, device="cuda"), torch.empty(m, 64, device="cuda")

        def gather():
            torch.index_select(o, 0, li, out=so)
            torch.index_select(hc, 0, li, out=sh)
            npg._pass(NPG_FVP, so, so, None, vec, hcache=sh, reduce=False)

        t_idx = timed(lambda: npg._pass_idx(o, idx, vec, hcache=hc))
        t_gat = timed(gather)
        t_plain = timed(lambda: npg._pass(NPG_FVP, so, so, None, vec, hcache=sh, reduce=False))
        lines.append(f"  frac {frac} ({m} rows): indexed pass {t_idx:.1f}; index_select x2 + plain pass {t_gat:.1f} "
                     f"(the plain pass on {m} gathered rows alone {t_plain:.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npgreg_time.txt"))
    ap.add_argument("--update-only", nargs=2)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("npgreg_time: no GPU (this tool measures on the device only)")
    if args.update_only:
        print(update_ms(args.root, float(args.update_only[0]), bool(int(args.update_only[1]))))
        return
    sys.path.insert(0, ROOT)
    lines = [f"NPG update with a subsampled Fisher and a BC term, {N} x {S} / {A}, 10 CG iterations "
             f"({torch.cuda.get_device_name(0)})", ""]
    pass_times(lines)
    lines += ["", f"whole update, ms (consecutive updates, each with its one host sync; {args.rounds} alternating rounds "
              "of fresh processes, every round listed):"]
    configs = [(1.0, False), (0.5, False), (0.25, False), (1.0, True), (0.5, True), (0.25, True)]
    res = {c: [] for c in configs}
    par = []
    for _ in range(args.rounds):
        if args.parent:
            par.append(child(args.parent, 1.0, False))
        for c in configs:
            res[c].append(child(ROOT, *c))
            print(f"[npgreg_time] frac {c[0]} bc {c[1]}: {res[c][-1]:.3f} ms", file=sys.stderr, flush=True)
    if args.parent:
        lines.append("  parent commit, frac 1, no BC:      " + "  ".join(f"{x:.3f}" for x in par))
    for (frac, bc), v in res.items():
        lines.append(f"  frac {frac:<4} {'BC ' + str(NE) + ' rows' if bc else 'no BC       '}:          " +
                     "  ".join(f"{x:.3f}" for x in v))
    # the restated fp32 torch loop on the host
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import npgreg_ref as G
    from amp_extensions_amd.npg import pack_policy
    from amp_extensions_amd.policy import init_mlp_policy_params
    torch.set_num_threads(args.threads)
    obs, act, adv, eo, ea = inputs()
    adv_w = (adv - adv.mean()) / (adv.std() + 1e-6)
    p0 = pack_policy(*init_mlp_policy_params(S, A, (32, 32), seed=100, init_log_std=-0.25))
    lines += ["", f"restated fp32 torch loop on the host (tests/npgreg_ref.py), {args.threads} threads, ms per update:"]
    for frac, bc in configs:
        idx = None if frac >= 0.99 else G.draws(0, N, frac)
        t0 = time.perf_counter()
        G.update(p0, S, A, obs, act, adv_w, idx=idx, bc=(eo, ea, REG) if bc else None)
        lines.append(f"  frac {frac:<4} {'BC' if bc else 'no BC'}: {(time.perf_counter() - t0) * 1e3:.0f}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
