"""Every entry point of csrc/amx_cost.hip against the plain CPU reference (tests/cost_ref.py):
the ordered fp64 partial sums, the witness, the per-row reward (separate and in the one-launch
relabel, at every width path of k_mmd_relabel), the expert cost with its two-batch pipeline,
the discriminator reward and the cost-input rows.

On exactly summable operands every output is compared bit for bit.  On real operands an output
is bit-equal wherever the fp64 dot cannot round to two fp32 values under the worst-case
summation bound (`near` false); a near row must take one of the two candidates.

test_ll_reward_accuracy measures the device's expf / log1pf against the longdouble value of
-logsigmoid; the allowed distance is twice the torch-CPU fp32 evaluation's own largest distance
on the same logits.  Measured on the MI355X over the 60 launches (device | torch-CPU fp32): largest
distance 2.27e-7 | 2.27e-7 (Hd = 512, 260 rows); the two differ in three launches only, and the
largest ratio device / CPU is 1.66 (4.78e-8 | 2.88e-8; Hd = 1, real rows).  DESIGN.md, parity section.
"""
import functools

import numpy as np
import pytest
import torch

import cost_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777.25
LAM, THR, CMIN, CMAX = C.LAM, C.THR, C.C_MIN, C.C_MAX
KINDS = ["exact", "real"]


@pytest.fixture(scope="module")
def env():
    import amp_extensions_amd as amx
    from amp_extensions_amd import _native as N
    ctx = amx.AmxContext(197, 36, n_models=4, hidden=512, n_hidden=4, feat_dim=512, device=DEV)
    yield ctx, N
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def stop_on_device_error():
    """A device error ends the session: nothing more is launched on a card that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def padded(rows, ld, extra=3):
    """[n + extra, ld] with NaN in the columns past the row width and in the extra rows."""
    rows = np.asarray(rows)
    out = np.full((rows.shape[0] + extra, ld), np.nan, rows.dtype)
    out[:rows.shape[0], :rows.shape[1]] = rows
    return dev(out)


def sent(n, dtype=torch.float32, extra=8):
    return torch.full((n + extra,), SENT, dtype=dtype, device=DEV)


def untouched(t, n):
    return bool((t[n:] == SENT).all().item())


def ptr(t):
    return None if t is None else t.data_ptr()


def check_rows(got, ref, lo, hi, near, n, exact, what):
    """got/ref/lo/hi: (reward, ipm, wb) triples (a None entry of got is skipped)."""
    alt_lo = np.ones(n, bool)
    alt_hi = np.ones(n, bool)
    for g, r, a, b in zip(got, ref, lo, hi):
        if g is None:
            continue
        assert untouched(g, n), f"{what}: wrote past n"
        g = g[:n].cpu().numpy()
        free = np.zeros(n, bool) if exact else near[:n]
        assert C.same_bits(g[~free], r[:n][~free]), f"{what}: differs from the reference"
        nan = np.isnan(g)
        alt_lo &= (C.bits(g) == C.bits(a[:n])) | (nan & np.isnan(a[:n]))
        alt_hi &= (C.bits(g) == C.bits(b[:n])) | (nan & np.isnan(b[:n]))
    if not exact:  # a near row takes one candidate dot in all three outputs
        assert np.all((alt_lo | alt_hi)[near[:n]]), f"{what}: a near row is off both candidates"


@functools.lru_cache(maxsize=None)
def reward_ref(kind, F):
    case = C.reward_case(kind, F)
    w, mmd, mlo, mhi, _ = C.mmd_fit(case["msg"], 0.0, case["phi_e"])
    refs = {}
    for clamp in (1, 0):
        lo, hi, near = C.reward_candidates(case["phi"], w, case["disc"], THR, LAM, CMIN, CMAX, clamp)
        ref = C.rewards(case["phi"], w, case["disc"], THR, LAM, CMIN, CMAX, clamp)[:3]
        refs[clamp] = (ref, lo, hi, near)
    return case, w, (mmd, mlo, mhi), refs


def launch_reward(env, clamp, phi_d, ld, w_d, F, disc_d, n, aux):
    ctx, N = env
    out = [sent(n), sent(n) if aux else None, sent(n) if aux else None]
    if clamp:
        N.check(ctx.lib.amx_mmd_reward(ctx.h, ptr(phi_d), ld, ptr(w_d), F, ptr(disc_d), THR, LAM, CMIN, CMAX,
                                       ptr(out[0]), ptr(out[1]), ptr(out[2]), n, ctx.stream), "reward")
    else:
        N.check(ctx.lib.amx_mmd_reward_raw(ctx.h, ptr(phi_d), ld, ptr(w_d), F, ptr(disc_d), LAM, ptr(out[0]),
                                           ptr(out[1]), ptr(out[2]), n, ctx.stream), "reward_raw")
    return out


def launch_relabel(env, clamp, msg_d, count, phi_e_d, F, phi_d, ld, disc_d, n, aux, erows_d=None, lde=0, n_e=0,
                   eout=None, emean=None, counter=None, erows_ptr=None):
    ctx, N = env
    out = [sent(n), sent(n) if aux else None, sent(n) if aux else None]
    w1, m1 = sent(F), sent(1)
    ep = erows_ptr if erows_ptr is not None else ptr(erows_d)
    N.check(ctx.lib.amx_mmd_relabel(ctx.h, ptr(msg_d), count, ptr(phi_e_d), F, ptr(w1), ptr(m1), ptr(phi_d), ld,
                                    ptr(disc_d), THR, LAM, clamp, CMIN, CMAX, ptr(out[0]), ptr(out[1]), ptr(out[2]), n,
                                    ep, lde, n_e, ptr(eout), ptr(emean), ptr(counter), ctx.stream), "relabel")
    return out, w1, m1


def check_fit(w1, m1, w, mmd3, F, exact, what):
    mmd, mlo, mhi = mmd3
    assert untouched(w1, F) and untouched(m1, 1), f"{what}: wrote past w / mmd"
    assert C.same_bits(w1[:F].cpu().numpy(), w), f"{what}: w"
    m = m1[:1].cpu().numpy()[0]
    assert (m == mmd) if exact else (m == mlo or m == mhi), f"{what}: w.w {m!r} vs {mmd!r} [{mlo!r}, {mhi!r}]"


@pytest.mark.parametrize("F", C.REWARD_F)
@pytest.mark.parametrize("kind", KINDS)
def test_reward_rows(env, kind, F):
    case, w, mmd3, refs = reward_ref(kind, F)
    exact = kind == "exact"
    w_d, phi_e_d, disc_d = dev(w), dev(case["phi_e"]), dev(case["disc"])
    msg_d = dev(case["msg"])
    msg_x = msg_d.clone()
    msg_x[F] = 12345.0  # with an explicit count the slot is not read
    assert (case["disc"] < THR).any() and (case["disc"] > THR).any()
    for ld in (F, F + 4):
        phi_d = padded(case["phi"], ld)
        phi_0 = phi_d.clone()
        for clamp in (1, 0):
            ref, lo, hi, near = refs[clamp]
            for n in C.REWARD_N:
                for aux in (True, False):
                    what = f"{kind} F={F} ld={ld} clamp={clamp} n={n} aux={aux}"
                    got = launch_reward(env, clamp, phi_d, ld, w_d, F, disc_d, n, aux)
                    check_rows(got, ref, lo, hi, near, n, exact, "separate " + what)
                    for m_d, count in ((msg_d, 0.0), (msg_x, case["count"])):
                        got, w1, m1 = launch_relabel(env, clamp, m_d, count, phi_e_d, F, phi_d, ld, disc_d, n, aux)
                        check_rows(got, ref, lo, hi, near, n, exact, f"fused count={count} " + what)
                        check_fit(w1, m1, w, mmd3, F, exact, f"fused count={count} " + what)
        assert C.same_bits(phi_d.cpu().numpy(), phi_0.cpu().numpy())


@pytest.mark.parametrize("F", [128, 512, 1152])
@pytest.mark.parametrize("clamp", [1, 0])
def test_row_isolation(env, clamp, F):
    """One NaN and one +inf in single phi entries of two rows and a NaN in one disc entry change
    those rows' outputs only, and these match the reference (NaN positions equal)."""
    n = 33
    case, w, _, _ = reward_ref("exact", F)
    phi, disc = case["phi"][:n].copy(), case["disc"][:n].copy()
    w_d, phi_e_d, msg_d = dev(w), dev(case["phi_e"]), dev(case["msg"])
    clean = launch_reward(env, clamp, dev(phi), F, w_d, F, dev(disc), n, True)
    clean = [c[:n].cpu().numpy() for c in clean]
    phi[3, 5], phi[17, F - 1], disc[20] = np.nan, np.inf, np.nan
    ref = C.rewards(phi, w, disc, THR, LAM, CMIN, CMAX, clamp)[:3]
    hit = np.zeros(n, bool)
    hit[[3, 17, 20]] = True
    phi_d, disc_d = dev(phi), dev(disc)
    fused = launch_relabel(env, clamp, msg_d, 0.0, phi_e_d, F, phi_d, F, disc_d, n, True)[0]
    for name, got in (("separate", launch_reward(env, clamp, phi_d, F, w_d, F, disc_d, n, True)), ("fused", fused)):
        for g, r, c in zip(got, ref, clean):
            assert untouched(g, n)
            g = g[:n].cpu().numpy()
            assert C.same_bits(g, r), f"{name}: differs from the reference"
            assert C.same_bits(g[~hit], c[~hit]), f"{name}: a clean row changed"
    assert np.isnan(ref[0][3]) and np.isnan(ref[0][20]) and not np.isnan(ref[0][17])


@functools.lru_cache(maxsize=2)
def expert_ref(kind, F, n_e):
    case = C.expert_case(kind, F, n_e)
    w, mmd, mlo, mhi, _ = C.mmd_fit(case["msg"], 0.0, case["phi_e"])
    return case, w, (mmd, mlo, mhi)


def run_expert(env, kind, F, case, w, mmd3, erows, erows_d, lde, row_off=0):
    """Separate and fused (three launches on one counter) expert cost of erows[row_off:]."""
    ctx, N = env
    exact = kind == "exact"
    rows = erows[row_off:]
    n_e = rows.shape[0]
    tot, mean, terms, near, bound = C.expert_cost(rows, w, LAM, CMIN, CMAX)
    ne = C.expert_blocks(n_e)
    eptr = erows_d.data_ptr() + row_off * lde * 4
    w_d, phi_e_d, msg_d, disc_d = dev(w), dev(case["phi_e"]), dev(case["msg"]), dev(case["disc"])
    n = case["phi"].shape[0]
    phi_d = dev(case["phi"])
    lo, hi, rnear = C.reward_candidates(case["phi"], w, case["disc"], THR, LAM, CMIN, CMAX, 1)
    ref = C.rewards(case["phi"], w, case["disc"], THR, LAM, CMIN, CMAX, 1)[:3]

    eo0, em0 = sent(1025, torch.float64), sent(1)
    N.check(ctx.lib.amx_expert_cost(ctx.h, eptr, lde, ptr(w_d), F, n_e, CMIN, CMAX, ptr(eo0), ptr(em0), LAM,
                                    ctx.stream), "expert")
    assert untouched(eo0, 1 + ne) and untouched(em0, 1)
    e0 = eo0[:1 + ne].cpu().numpy()
    m0 = em0[:1].cpu().numpy()[0]
    print(f"expert {kind} F={F} n_e={n_e} off={row_off}: sum {e0[0]!r} ref {tot!r} |diff| {abs(e0[0] - tot):.3e} "
          f"bound {bound:.3e} near rows {int(near.sum())}")
    if exact:
        assert e0[0] == tot and C.same_bits(np.float32(m0), np.float32(mean)), (e0[0], tot, m0, mean)
        assert np.array_equal(e0[1:], C.expert_partials(terms)), "block partials"
    else:
        assert abs(e0[0] - tot) <= bound, (e0[0], tot, bound)
        assert C.same_bits(np.float32(m0), C.expert_mean(e0[0], n_e, LAM))
    counter = torch.zeros(4, dtype=torch.int32, device=DEV)
    for it in range(3):
        eo1, em1 = sent(1025, torch.float64), sent(1)
        got, w1, m1 = launch_relabel(env, 1, msg_d, 0.0, phi_e_d, F, phi_d, F, disc_d, n, True, lde=lde, n_e=n_e,
                                     eout=eo1, emean=em1, counter=counter, erows_ptr=eptr)
        assert int(counter[0].item()) == 0, f"launch {it}: counter not reset"
        assert untouched(eo1, 1 + ne) and untouched(em1, 1)
        assert C.same_bits(eo1[:1 + ne].cpu().numpy(), e0), f"launch {it}: fused sum / block partials"
        assert C.same_bits(em1[:1].cpu().numpy(), np.array([m0])), f"launch {it}: fused mean"
        check_rows(got, ref, lo, hi, rnear, n, exact, f"fused with expert rows, launch {it}")
        check_fit(w1, m1, w, mmd3, F, exact, f"fused with expert rows, launch {it}")


@pytest.mark.parametrize("F,n_e", C.EXPERT_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_expert_cost(env, kind, F, n_e):
    case, w, mmd3 = expert_ref(kind, F, n_e)
    small = n_e < 4096
    lde = F + 4 if small else F
    erows_d = padded(case["erows"], lde, extra=3 if small else 0)
    run_expert(env, kind, F, case, w, mmd3, case["erows"], erows_d, lde)


@pytest.mark.parametrize("kind", KINDS)
def test_expert_cost_sharded(env, kind):
    """The sharded form: the expert pointer offset by a whole number of rows."""
    F, n_e = 512, 16385
    case, w, mmd3 = expert_ref(kind, F, n_e)
    erows_d = dev(case["erows"])
    run_expert(env, kind, F, case, w, mmd3, case["erows"], erows_d, F, row_off=4099)


def test_expert_cost_rejects_misaligned_rows(env):
    """row_dot loads float4: rows or w off a 16-byte boundary are refused on the host."""
    ctx, N = env
    buf, w = torch.zeros(4 * 132 + 4, device=DEV), torch.zeros(132, device=DEV)
    out, mean = sent(1025, torch.float64), sent(1)
    for rows_p, w_p in ((buf.data_ptr() + 4, w.data_ptr()), (buf.data_ptr(), w.data_ptr() + 4)):
        rc = ctx.lib.amx_expert_cost(ctx.h, rows_p, 128, w_p, 128, 4, CMIN, CMAX, ptr(out), ptr(mean), LAM, ctx.stream)
        assert rc != 0 and b"aligned" in ctx.lib.amx_last_error()
    torch.cuda.synchronize()
    assert untouched(out, 0) and untouched(mean, 0)


@pytest.mark.parametrize("F", C.PARTS_F)
@pytest.mark.parametrize("n_parts", C.PARTS_N)
def test_partial_sums(env, n_parts, F):
    ctx, N = env
    parts = C.int_parts(n_parts, F, n_parts + F)
    ref = C.colsum(parts, F)
    assert np.array_equal(ref, parts.sum(0))  # integer-valued: any order is exact
    parts_d = dev(parts) if n_parts else torch.zeros(1, dtype=torch.float64, device=DEV)
    out = sent(F, torch.float64)
    N.check(ctx.lib.amx_sum_partials(ctx.h, ptr(parts_d), n_parts, F, ptr(out), ctx.stream), "sum")
    assert untouched(out, F) and C.same_bits(out[:F].cpu().numpy(), ref)
    msg = sent(F + 1, torch.float64)
    N.check(ctx.lib.amx_feature_message(ctx.h, ptr(parts_d), n_parts, F, 40960.0, ptr(msg), ctx.stream), "msg")
    assert untouched(msg, F + 1) and C.same_bits(msg[:F + 1].cpu().numpy(), np.concatenate([ref, [40960.0]]))


@pytest.mark.parametrize("F", C.FIT_F)
@pytest.mark.parametrize("kind", KINDS)
def test_mmd_fit(env, kind, F):
    ctx, N = env
    case = C.make_case(kind, F, 64, 64, 2)
    w, mmd, mlo, mhi, _ = C.mmd_fit(case["msg"], 0.0, case["phi_e"])
    phi_e_d, msg_d = dev(case["phi_e"]), dev(case["msg"])
    msg_x = msg_d.clone()
    msg_x[F] = 12345.0
    for m_d, count in ((msg_d, 0.0), (msg_x, case["count"])):
        w1, m1 = sent(F), sent(1)
        N.check(ctx.lib.amx_mmd_fit(ctx.h, ptr(m_d), count, ptr(phi_e_d), F, ptr(w1), ptr(m1), ctx.stream), "fit")
        check_fit(w1, m1, w, (mmd, mlo, mhi), F, kind == "exact", f"fit {kind} F={F} count={count}")


def launch_disc(env, loss, h_d, ldh, Hd, w3_d, b3, disc_d, n, want_logits):
    ctx, N = env
    reward, logits = sent(n), sent(n) if want_logits else None
    N.check(ctx.lib.amx_disc_reward(ctx.h, loss, ptr(h_d), ldh, Hd, ptr(w3_d), b3, ptr(disc_d), LAM, ptr(reward),
                                    ptr(logits), n, ctx.stream), "disc_reward")
    assert untouched(reward, n) and (logits is None or untouched(logits, n))
    return reward[:n].cpu().numpy(), None if logits is None else logits[:n].cpu().numpy()


def head_logits(env, kind, Hd, b3, loss, case, h_d, w3_d, n):
    """The device logits of the first n rows, checked against the reference's."""
    lo, hi, near = C.logit_candidates(case["h"][:n], case["w3"], b3)
    _, D = launch_disc(env, loss, h_d, Hd + 3, Hd, w3_d, b3, None, n, True)
    if kind == "exact":
        assert C.same_bits(D, C.disc_reward(case["h"][:n], case["w3"], b3, 0, None, LAM)[1])
        if b3 == 0.0:
            k = min(n, len(C.HEAD_LOGITS))
            assert np.array_equal(D[:k], np.array(C.HEAD_LOGITS[:k], np.float32))
    else:
        assert C.same_bits(D[~near], lo[~near])
        assert np.all((C.bits(D) == C.bits(lo)) | (C.bits(D) == C.bits(hi)))
    return D


@pytest.mark.parametrize("Hd", C.HEAD_HD)
@pytest.mark.parametrize("kind", KINDS)
def test_disc_reward_least_squares(env, kind, Hd):
    case = C.make_head(kind, Hd, C.HEAD_ROWS, 0)
    h_d, w3_d, disc_d = padded(case["h"], Hd + 3), dev(case["w3"]), dev(case["disc"])
    for b3 in (0.0, 0.375):
        for n in C.HEAD_N:
            D = head_logits(env, kind, Hd, b3, 0, case, h_d, w3_d, n)
            for dd, dn in ((None, None), (disc_d, case["disc"][:n])):
                ref = C.disc_algebra(D, 0, dn, LAM)[0]  # the fp32 algebra is exact given the logits
                for want in (True, False):
                    r, D2 = launch_disc(env, 0, h_d, Hd + 3, Hd, w3_d, b3, dd, n, want)
                    assert C.same_bits(r, ref), f"{kind} Hd={Hd} b3={b3} n={n} disc={dn is not None}"
                    assert D2 is None or C.same_bits(D2, D)


@pytest.mark.parametrize("Hd", C.HEAD_HD)
@pytest.mark.parametrize("kind", KINDS)
def test_ll_reward_accuracy(env, kind, Hd):
    """Log-likelihood reward: expf / log1pf on the device need not match libm bit for bit.  The
    device's distance from the longdouble value of -(min(D,0) - log1p(exp(-|D|))) may be at most
    twice the torch-CPU fp32 evaluation's own largest distance on the same logits (one more
    rounding in each of the two transcendental calls)."""
    case = C.make_head(kind, Hd, C.HEAD_ROWS, 0)
    h_d, w3_d, disc_d = padded(case["h"], Hd + 3), dev(case["w3"]), dev(case["disc"])
    for b3 in (0.0, 0.375):
        for n in C.HEAD_N:
            D = head_logits(env, kind, Hd, b3, 1, case, h_d, w3_d, n)
            exactv = C.ll_reward_ld(D)
            e_cpu = float(np.abs(C.ll_reward_f32(D).astype(C.LD) - exactv).max())
            rew, _ = launch_disc(env, 1, h_d, Hd + 3, Hd, w3_d, b3, None, n, False)
            e_dev = float(np.abs(rew.astype(C.LD) - exactv).max())
            print(f"ll {kind} Hd={Hd} b3={b3} n={n}: device max |err| {e_dev:.3e}, torch-CPU fp32 {e_cpu:.3e}")
            assert e_dev <= 2.0 * e_cpu, (e_dev, e_cpu)
            # the algebra around the loss term, bit for bit on the device's own term
            r2, D2 = launch_disc(env, 1, h_d, Hd + 3, Hd, w3_d, b3, None, n, True)
            assert C.same_bits(r2, rew) and C.same_bits(D2, D)
            ref = C.disc_algebra(D, 1, case["disc"][:n], LAM, rew=rew)[0]
            for want in (True, False):
                r3, _ = launch_disc(env, 1, h_d, Hd + 3, Hd, w3_d, b3, disc_d, n, want)
                assert C.same_bits(r3, ref)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("widths", [(5, 0, 3), (0, 4, 2), (7, 3, 0), (0, 0, 6), (197, 36, 197)])
def test_cost_rows(env, widths, B):
    ctx, N = env
    rs = np.random.RandomState(sum(widths) + B)
    segs, segs_d, args = [], [], []
    for wd in widths:
        ld = wd + 3
        x = rs.randn(B + 1, ld) * 10.0 ** rs.randint(-3, 4, (B + 1, ld))
        x[0, :2] = [1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50]  # a tie to even, and just above it
        x[:, wd:] = np.nan
        x_d = dev(x) if wd else None
        segs.append(x[:B])
        segs_d.append(x_d)
        args += [ptr(x_d), ld if wd else 0, wd]
    ldc = sum(widths) + 5
    ref = C.cost_rows(segs, widths, ldc)
    out = torch.full(((B + 2) * ldc,), SENT, dtype=torch.float32, device=DEV)
    N.check(ctx.lib.amx_cost_rows(ctx.h, *args, B, ptr(out), ldc, ctx.stream), "cost_rows")
    assert untouched(out, B * ldc)
    got = out[:B * ldc].cpu().numpy().reshape(B, ldc)
    assert C.same_bits(got, ref) and np.array_equal(got[:, sum(widths):], np.zeros((B, 5), np.float32))
