"""Time the DTW evaluation score (csrc/amx_dtw.hip) and write profiles/dtw_time.txt:
  * us per amx_dtw_align launch (the scene's cell cost, TimeWarpCost; the squared DefaultCost
    beside it) for 20 and for 256 trajectories of length 301 at dim 45 in a 302 buffer (HIP events
    around REPS back-to-back launches, after a warm-up), and per TimeWarper.score call (rows from
    states, rows from the clip, the alignment) for 20;
  * the host restatement (tests/dtw_ref.py align with TimeWarpCost: numpy distances, the
    recurrence and the backtrack as Python loops, one thread) on the first HOST_N of the same trajectories, on the
    same box, and that its costs agree with the device's.
The rows are the kinematic character's from random clip times against themselves + 0.02 N(0, 1),
the alignment of a rollout that tracks the clip.  Reported, not gated.
usage: python tools/dtw_time.py"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import amp_extensions_amd as amx  # noqa: E402
import dtw_ref as R  # noqa: E402
from amp_extensions_amd.motion import ReferenceMotion  # noqa: E402

S, A, LEN, REPS, HOST_N = 226, 28, 301, 20, 4
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
    ctx = amx.AmxContext(S, A, n_models=4, hidden=64, n_hidden=4, device=DEV)
    rm = ReferenceMotion.from_bundle(ctx)
    tw = amx.TimeWarper(ctx, rm)
    n_max, dim = tw.buffer_size, tw.dim
    props = torch.cuda.get_device_properties(0)
    say(f"DTW score: trajectories of {LEN} rows, dim {dim}, buffer {n_max}, cell cost TimeWarpCost; device {props.name}, "
        f"{props.multi_processor_count} CUs; {REPS} launches per figure")
    rs = np.random.RandomState(0)
    host = None
    for T in (20, 256):
        t0 = rs.uniform(0, rm.duration, T)
        kin = tw.rows_from_motion(t0, n_max)
        sim = kin + 0.02 * torch.from_numpy(rs.randn(T, n_max, dim)).to(DEV)
        lens = [LEN] * T
        us = timed(lambda: tw.align(sim, kin, lens, buffer_size=n_max))
        out = tw.align(sim, kin, lens, buffer_size=n_max)
        say(f"amx_dtw_align, {T:3d} trajectories in one launch (TimeWarper.align, output allocation included): "
            f"{us:9.1f} us  ({us / T:7.1f} us per trajectory)")
        us2 = timed(lambda: tw.align(sim, kin, lens, buffer_size=n_max, cost="squared"))
        say(f"  the same with the squared DefaultCost: {us2:9.1f} us")
        if host is None:
            a, b = sim[:HOST_N, :LEN].cpu().numpy(), kin[:HOST_N, :LEN].cpu().numpy()
            t1 = time.perf_counter()
            ref = [R.align(a[k], b[k], n_max) for k in range(HOST_N)]
            host = (time.perf_counter() - t1) / HOST_N
            got = out["dtw_cost"][:HOST_N].cpu().numpy()
            err = max(abs(got[k] - ref[k]["dtw_cost"]) / ref[k]["dtw_cost"] for k in range(HOST_N))
            same = all((out["index"][k, :LEN].cpu().numpy() == ref[k]["index"]).all() for k in range(HOST_N))
            states = rm.states(t0)
            sl = [states[k:k + 1].expand(LEN, S) for k in range(T)]
            us_score = timed(lambda: tw.score(sl, t0), reps=5, warm=1)
            say(f"TimeWarper.score, {T} trajectories of {LEN} states (state rows + clip rows + alignment): "
                f"{us_score:9.1f} us")
    say(f"host restatement (tests/dtw_ref.py align, TimeWarpCost: numpy {np.__version__} distances, Python-loop recurrence and "
        f"backtrack, one thread), same trajectories, same box: {host * 1e3:7.1f} ms per trajectory "
        f"(mean of {HOST_N}; {host * 20:.1f} s for 20, {host * 256:.0f} s for 256 at that rate); "
        f"dtw_cost max relative difference to the device {err:.1e}, index paths equal: {same}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dtw_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
