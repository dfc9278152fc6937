"""The step kernels (csrc/amx_step.hip: step_lane in k_step<NIT, MM4> and k_step_act<NIT, MM4, W8>)
against G21, the reference's own SimEnv.is_done (tests/golden/make_golden_term.py), at every
state width NIT = ceil(S / 64) = 1..8, on the four-member fast path and the generic member loop,
under every record / velocity flag combination and over fall-body tables of 0, 1, 6, 13 and 32
bodies (tests/term_cases.py).  One context per (case, member count); all calls go through the
C ABI.

Bit-exact: done, num_steps, ob_next (the fp64 of the fp32 -> fp64 add, with G21's rescaled
velocity block where check_velocity mutates it), the cost-input rows, the non-finite flags, the
reset bookkeeping, and the fused policy against the stand-alone one.  The disagreement is
compared with the fp64 computation the kernel documents (fp32 pair differences, fp64 sum of
squares, sqrt, rounded to fp32) within 1 fp32 ulp: only the fp64 summation order differs
(~1e-16 relative), so the rounded value can move only at a rounding tie.

Instantiations launched (NIT by case: s40 1, s100 2, s150 3, s197 4, s300 5, s350 6, s420 7,
s512 8): k_step<1..8, true> by M = 4 and k_step<1..8, false> by M = 2 (plus M = 8 at NIT 2 and
M = 1 at NIT 6) through amx_step and amx_step_reset (amx_step_rexp at NIT 4 and 7);
k_step_act<1..4, true, false>, <1..4, true, true> and <1..4, false, false> through
amx_step_reset_act."""
import numpy as np
import pytest
import torch

import term_cases as T
from oracle import milo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x5EED5EED

STEP_PARAMS = [(n, m) for n in T.CASE_NAMES for m in (4, 2)] + [("s100", 8), ("s350", 1)]
ACT_CASES = [n for n in T.CASE_NAMES if T.CASES[n]["S"] <= 256]


@pytest.fixture(scope="module")
def g21(golden):
    return golden("g21_termination.npz")


@pytest.fixture(scope="module")
def contexts():
    import amp_extensions_amd as amx
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    cache = {}

    def get(name, M):
        if (name, M) not in cache:
            spec = T.CASES[name]
            S, A = spec["S"], spec["A"]
            ctx = amx.AmxContext(S, A, n_models=M, hidden=16, n_hidden=1, feat_dim=128, device=DEV)
            rs = np.random.RandomState(S + M)
            ctx.set_normalizers([torch.from_numpy(x.astype(np.float32)) for x in (
                0.1 * rs.randn(S), rs.uniform(0.5, 2.0, S), 0.1 * rs.randn(A), rs.uniform(0.5, 2.0, A),
                np.zeros(S), np.ones(S))])
            cache[name, M] = ctx
        return cache[name, M]

    return get


def term_config(spec, cfg):
    from amp_extensions_amd.humanoid import TerminationConfig
    return TerminationConfig(fall_bodies=tuple(spec["fall_bodies"]), body_defs=dict(spec["body_defs"]),
                             pos_dim=spec["pos_dim"], rot_dim=spec["rot_dim"], horizon=T.HORIZON,
                             vel_offset=spec["vel_offset"], vel_threshold=T.VEL_THRESHOLD,
                             sampling_rate=T.SAMPLING_RATE, **T.config_flags(cfg))


def member_inputs(c, M):
    """A random member per lane; member m's predictions are `pred` shifted by (m - member) * 1e-3, so
    stepping with the wrong member flips `done` on the boundary rows."""
    B = c["ob"].shape[0]
    rs = np.random.RandomState(9 + M)
    k = rs.randint(0, M, B).astype(np.int32)
    preds = np.stack([c["pred"] + (m - k[:, None]).astype(np.float32) * np.float32(0.001) for m in range(M)])
    preds[k, np.arange(B)] = c["pred"]
    return k, np.ascontiguousarray(preds, dtype=np.float32)


def expected(c, cfg, g21):
    """(ob_next, done, num_steps, nonfinite) of G21 for a configuration."""
    vo = c["spec"]["vel_offset"]
    nxt = c["ob"] + c["pred"].astype(np.float64)  # IEEE: the kernel's o + (double)p
    f = T.config_flags(cfg)
    if f["enable_velocity_check"] and f["record_vel_as_pos"]:
        nxt[:, vo:] = g21[f"{c['name']}__vel"]
    return nxt, g21[f"{c['name']}__{cfg}__done"], c["num_steps"] + 1, (~np.isfinite(nxt).all(1)).astype(np.uint8)


def disc_reference(preds):
    """max over pairs of ||p_i - p_k||: fp32 differences, fp64 sum of squares, sqrt, rounded to fp32."""
    M = preds.shape[0]
    best = None
    for i in range(M):
        for k in range(i + 1, M):
            d = (preds[i] - preds[k]).astype(np.float64)
            n = (d * d).sum(1)
            best = n if best is None else np.maximum(best, n)
    return np.sqrt(best).astype(np.float32)


def assert_within_one_ulp(got, ref):
    assert (got >= 0).all() and np.isfinite(got).all()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, (int(ulps.max()), int(ulps.argmax()))


def row_exponents(ci):
    """Smallest e with max|row| < 2^e, clamped to [-100, 100] (a non-finite row takes the clamp)."""
    mx = np.abs(ci).max(1)
    fin = np.isfinite(mx)
    e = np.frexp(np.where(fin, mx, 1.0))[1]
    return np.clip(np.where(fin, e, 100), -100, 100).astype(np.int32)


class Lanes:
    """Device buffers of one step launch, pre-filled with values no kernel writes."""

    def __init__(self, ctx, c, M, ldc, in_place=False):
        B, S = c["ob"].shape
        self.ctx, self.c, self.M, self.B, self.S, self.ldc = ctx, c, M, B, S, ldc
        self.k, self.preds_h = member_inputs(c, M)
        rs = np.random.RandomState(21)
        self.table_h = rs.randn(5, S)
        self.rows_h = rs.randint(0, 5, B).astype(np.int32)
        self.rc_h = rs.randint(0, 9, B).astype(np.int32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)
        self.preds, self.model_idx, self.ob = t(self.preds_h), t(self.k), t(c["ob"])
        self.ns, self.table, self.rows, self.rc = t(c["num_steps"]), t(self.table_h), t(self.rows_h), t(self.rc_h)
        self.nxt = f((B, S), -7.0, torch.float64)
        self.done = f((B,), 9, torch.uint8)
        self.nonfinite = f((B,), 9, torch.uint8)
        self.disc = f((B,), -1.0, torch.float32) if M >= 2 else None
        self.cost_in = f((B, ldc), 7.0, torch.float32)
        self.rexp = f((B,), 77, torch.int32)
        self.ob_out = self.ob if in_place else f((B, S), -7.0, torch.float64)
        self.ob_rec = f((B, S), -7.0, torch.float64)
        self.row_out = f((B,), 77, torch.int32)
        self.steps0 = f((B,), 77, torch.int32)

    def head(self):
        p = lambda x: None if x is None else x.data_ptr()
        return (self.ctx.h, p(self.preds), self.S, self.B * self.S, p(self.model_idx), p(self.ob), p(self.nxt),
                p(self.ns), p(self.done), p(self.disc), p(self.cost_in), self.ldc)

    def reset_args(self):
        return (self.table.data_ptr(), 5, self.rows.data_ptr(), SEED, self.ob_out.data_ptr(), self.rc.data_ptr(),
                self.row_out.data_ptr(), self.steps0.data_ptr())

    def check_step(self, cfg, g21, rexp=False):
        c, S = self.c, self.S
        nxt, done, ns, nonf = expected(c, cfg, g21)
        np.testing.assert_array_equal(self.done.cpu().numpy(), done, err_msg=cfg)
        np.testing.assert_array_equal(self.nxt.cpu().numpy(), nxt, err_msg=cfg)
        np.testing.assert_array_equal(self.nonfinite.cpu().numpy(), nonf, err_msg=cfg)
        ci = self.cost_in.cpu().numpy()
        np.testing.assert_array_equal(ci[:, :2 * S], np.concatenate([c["ob"], nxt], 1).astype(np.float32))
        assert (ci[:, 2 * S:] == 0).all() and ci.shape[1] == self.ldc
        if self.M >= 2:
            assert_within_one_ulp(self.disc.cpu().numpy(), disc_reference(self.preds_h))
        if rexp:
            np.testing.assert_array_equal(self.rexp.cpu().numpy(), row_exponents(ci[:, :2 * S]))
        return nxt, done, ns

    def check_reset(self, cfg, g21, in_place=False, rexp=True):
        nxt, done, ns, = self.check_step(cfg, g21, rexp=rexp)
        d = done.astype(bool)
        np.testing.assert_array_equal(self.ob_out.cpu().numpy(), np.where(d[:, None], self.table_h[self.rows_h], nxt))
        np.testing.assert_array_equal(self.rc.cpu().numpy(), self.rc_h + d)
        np.testing.assert_array_equal(self.model_idx.cpu().numpy(), np.where(d, (self.rc_h + 1) % self.M, self.k))
        np.testing.assert_array_equal(self.ns.cpu().numpy(), np.where(d, 0, ns))
        np.testing.assert_array_equal(self.row_out.cpu().numpy(), np.where(d, self.rows_h, -1))
        np.testing.assert_array_equal(self.steps0.cpu().numpy(), self.c["num_steps"])
        if not in_place:
            np.testing.assert_array_equal(self.ob.cpu().numpy(), self.c["ob"])
            np.testing.assert_array_equal(self.ob_rec.cpu().numpy(), self.c["ob"])


@pytest.mark.parametrize("name,M", STEP_PARAMS)
def test_step_matches_reference_is_done(contexts, g21, name, M):
    """amx_step under every configuration of the case; once with a deliberately over-wide ldc."""
    from amp_extensions_amd import _native as N
    ctx, c = contexts(name, M), T.load_case(name, g21)
    for i, cfg in enumerate(c["spec"]["configs"]):
        ctx.set_termination(term_config(c["spec"], cfg))
        L = Lanes(ctx, c, M, ldc=ctx.k_rff_pad + (96 if i == 0 else 0))
        N.check(ctx.lib.amx_step(*L.head(), L.nonfinite.data_ptr(), L.B, ctx.stream), "amx_step")
        _, _, ns = L.check_step(cfg, g21)
        np.testing.assert_array_equal(L.ns.cpu().numpy(), ns)
        np.testing.assert_array_equal(L.model_idx.cpu().numpy(), L.k)


def test_step_without_disagreement_single_member(contexts, g21):
    """M = 1: disc is null and the call succeeds (a non-null disc is refused)."""
    from amp_extensions_amd import _native as N
    ctx, c = contexts("s350", 1), T.load_case("s350", g21)
    ctx.set_termination(term_config(c["spec"], "a0r0v0"))
    L = Lanes(ctx, c, 1, ldc=ctx.k_rff_pad)
    assert L.disc is None
    bad = torch.zeros(L.B, dtype=torch.float32, device=DEV)
    head = list(L.head())
    head[9] = bad.data_ptr()
    assert ctx.lib.amx_step(*head, L.nonfinite.data_ptr(), L.B, ctx.stream) == -1  # AMX_E_INVAL
    head[9] = None
    N.check(ctx.lib.amx_step(*head, L.nonfinite.data_ptr(), L.B, ctx.stream), "amx_step")
    L.check_step("a0r0v0", g21)


def test_body_inside_rescaled_velocity_block_is_refused(contexts):
    """check_collision reads ob before check_velocity's in-place rescale (sim_env.py:171-172); the
    kernel rescales first, so amx_set_termination refuses a checked body element at or past
    vel_offset when the rescale is on (no real layout has one: the pose block comes first)."""
    from amp_extensions_amd import _native as N
    ctx = contexts("s100", 2)
    spec = dict(T.CASES["s100"], vel_offset=50)  # body 8's normal y = 52, body 10's y = 62
    with pytest.raises(N.AmxNativeError, match="velocity block"):
        ctx.set_termination(term_config(spec, "a0r0v2"))
    ctx.set_termination(term_config(spec, "a0r0v1"))  # no rescale: nothing to refuse


@pytest.mark.parametrize("name,M", [("s197", 4), ("s420", 2)])
def test_step_rexp_row_exponents(contexts, g21, name, M):
    from amp_extensions_amd import _native as N
    ctx, c = contexts(name, M), T.load_case(name, g21)
    for cfg in c["spec"]["configs"][:3]:
        ctx.set_termination(term_config(c["spec"], cfg))
        L = Lanes(ctx, c, M, ldc=ctx.k_rff_pad)
        N.check(ctx.lib.amx_step_rexp(*L.head(), L.rexp.data_ptr(), L.nonfinite.data_ptr(), L.B, ctx.stream),
                "amx_step_rexp")
        L.check_step(cfg, g21, rexp=True)
    e = L.rexp.cpu().numpy()
    assert e.max() == 100 and len(np.unique(e)) >= 3  # the non-finite clamp and several exponents occur


@pytest.mark.parametrize("name,M", STEP_PARAMS)
def test_step_reset_matches_reference_is_done(contexts, g21, name, M):
    """amx_step_reset with injected rows: the step outputs unchanged, done lanes restart from the
    table (sim_env.py:270-285); the first configuration runs in place (ob_out == ob)."""
    from amp_extensions_amd import _native as N
    ctx, c = contexts(name, M), T.load_case(name, g21)
    for i, cfg in enumerate(c["spec"]["configs"]):
        ctx.set_termination(term_config(c["spec"], cfg))
        L = Lanes(ctx, c, M, ldc=ctx.k_rff_pad, in_place=i == 0)
        N.check(ctx.lib.amx_step_reset(*L.head(), L.rexp.data_ptr(), L.nonfinite.data_ptr(), *L.reset_args(), None, 0,
                                       None if i == 0 else L.ob_rec.data_ptr(), L.B, ctx.stream), "amx_step_reset")
        L.check_reset(cfg, g21, in_place=i == 0)


@pytest.mark.parametrize("name,M,w8", [(n, m, w) for n in ACT_CASES for m, w in ((4, 0), (4, 1), (2, 0))])
def test_step_reset_act_matches_step_reset_and_policy(contexts, g21, name, M, w8):
    """amx_step_reset_act: every step output as G21 (and so as amx_step_reset), and act, mean, the
    x0 rows and the row exponents equal amx_policy_act on the ob_out it produced -- the identity
    include/amx_hip.h promises -- with a 32 x 32 policy packed by amx_policy_pack."""
    import amp_extensions_amd as amx
    from amp_extensions_amd import _native as N
    ctx, c = contexts(name, M), T.load_case(name, g21)
    S, A = c["spec"]["S"], c["spec"]["A"]
    pw, log_std = R.init_policy_weights(S, A, (32, 32), seed=100, init_log_std=-0.25)
    pol = amx.DevicePolicy(ctx, pw, log_std, seed=3)
    N.check(ctx.lib.amx_set_step_act_occupancy(ctx.h, w8), "amx_set_step_act_occupancy")
    try:
        for cfg in c["spec"]["configs"][:3]:
            ctx.set_termination(term_config(c["spec"], cfg))
            L = Lanes(ctx, c, M, ldc=ctx.k_rff_pad)
            B, Bp = L.B, (L.B + 127) // 128 * 128
            outs = []
            for fused in (True, False):
                act = torch.full((B, A), -7.0, dtype=torch.float64, device=DEV)
                mean = torch.full((B, A), -7.0, dtype=torch.float32, device=DEV)
                x0 = torch.full((Bp, ctx.ldk), 7.0, dtype=torch.float32, device=DEV)
                rx = torch.full((M, 2, Bp), 77, dtype=torch.int32, device=DEV)
                tail = (act.data_ptr(), mean.data_ptr(), x0.data_ptr(), 0, ctx.ldk, rx.data_ptr(), rx.stride(0),
                        rx.stride(1), 2)
                if fused:
                    N.check(ctx.lib.amx_step_reset_act(
                        *L.head(), L.rexp.data_ptr(), L.nonfinite.data_ptr(), *L.reset_args(), L.ob_rec.data_ptr(),
                        pol.blob.data_ptr(), pol.H1, pol.H2, pol.noise_scale.data_ptr(), pol.seed, 11, None, 0, *tail,
                        B, ctx.stream), "amx_step_reset_act")
                else:
                    N.check(ctx.lib.amx_policy_act(
                        ctx.h, L.ob_out.data_ptr(), B, pol.blob.data_ptr(), pol.H1, pol.H2,
                        pol.noise_scale.data_ptr(), None, pol.seed, 11, 0, *tail, ctx.stream), "amx_policy_act")
                outs.append((act, mean, x0, rx))
            L.check_reset(cfg, g21)
            for nm, a, b in zip(("act", "mean", "x0", "row_exp"), *outs):
                torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=f"{cfg}: {nm}")
            act = outs[0][0].cpu().numpy()
            fin = np.isfinite(L.ob_out.cpu().numpy()).all(1)
            assert np.isfinite(act[fin]).all() and (act[fin] != -7.0).all() and (outs[0][3][:, 0, :B] != 77).all()
    finally:
        ctx.lib.amx_set_step_act_occupancy(ctx.h, 0)
