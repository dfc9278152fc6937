"""Every ensemble GEMM tile family, one launch of its C entry point per case, bit for bit against
the numpy restatement of tests/h3_exact.py on operands for which the f16x3 sum (and the f32 and
bf16x6 sums) are exact in fp32 in any order: np.array_equal, no tolerance.  A mismatch is a
kernel, split or dispatch bug (or a branch pick_tile restates wrongly); the failing rows, columns
and K tell which stage.

Each case also checks: the weight image's limbs and exponents against numpy, the row-exponent
kernel, the shared-x0 select (the other members' leading columns hold NaN), NaN in the operands'
row padding, an all-zero A row (the result is the bias alone), sentinels around the written
slice (col_off / ldc, ldp > S, columns >= S), the hidden layers' row-exponent output, zeroed
stream-K counters over a NaN-filled scratch, and the same bytes from a second launch."""
import numpy as np
import pytest
import torch

import h3_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def contexts():
    import amp_extensions_amd as amx
    made = {}

    def get(S):
        if S not in made:
            ctx = amx.AmxContext(S, X.A_DIM, n_models=4, hidden=512, n_hidden=4, feat_dim=512, device=DEV)
            ctx.set_normalizers(X.normalizers(S))
            made[S] = ctx
        return made[S]

    return get


def same(got, want, what):
    """np.array_equal (zeros of either sign equal as values), with the failing pattern spelled out."""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    axes = ["member", "row", "column"][-bad.shape[1]:]
    spread = ", ".join(f"{len(np.unique(bad[:, i]))} {a}s [{bad[:, i].min()}..{bad[:, i].max()}]"
                       for i, a in enumerate(axes))
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}" for i in bad[:6])
    pytest.fail(f"{what}: {len(bad)} of {got.size} elements differ ({spread}); {first}")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_tile_is_exact(contexts, case):
    from amp_extensions_amd import _native as N
    c = case
    ctx = contexts(c.S)
    if ctx.n_cus != X.N_CUS:
        pytest.skip(f"the case table is derived for {X.N_CUS} compute units (MI355X); this device has {ctx.n_cus}")
    assert X.pick_tile(ctx.n_cus, c.epi, c.groups, c.rows, c.N, c.K, c.S, c.ws) == c.family
    lib, h, st = ctx.lib, ctx.h, ctx.stream
    G, rows, Nw, K, ks = c.groups, c.rows, c.N, c.K, c.k_shared
    hidden = c.epi.startswith("hidden")
    inp = X.case_inputs(c)
    assert X.case_bound(c) < 2.0 ** 22
    want, want_exp = X.expected(c, inp)
    ld = K + X.LD_PAD
    A, Wd, bias = dev(inp["A_dev"]), dev(inp["W_dev"]), dev(inp["bias"])
    sA, sW = rows * ld, Nw * ld

    # ---- operands: the weight image and the row exponents
    if c.path == "h3":
        W2 = torch.empty(G, Nw, 2 * K, dtype=torch.int16, device=DEV)
        wexp = torch.empty(G, Nw, dtype=torch.int32, device=DEV)
        N.check(lib.amx_split_f16x2(h, G, Nw, K, Wd.data_ptr(), ld, sW, W2.data_ptr(), Nw * 2 * K, wexp.data_ptr(),
                                    Nw, st), "amx_split_f16x2")
        Ec = X.row_exponent(inp["W"])
        hi, lo = X.split_limbs(inp["W"], Ec)
        limbs = W2.cpu().numpy().view(np.uint16).reshape(G, Nw, K // 16, 2, 16)
        for i, (name, ref) in enumerate((("hi", hi), ("lo", lo))):
            same(limbs[:, :, :, i, :].reshape(G, Nw, K), ref.astype(np.float16).view(np.uint16), f"W image {name} limb bits")
        same(wexp.cpu().numpy(), Ec.astype(np.int32), "w_exp")
        in_slots = 2 if ks else 1
        slots = in_slots + (1 if hidden else 0)
        rexp = torch.full((G, slots, rows), 77, dtype=torch.int32, device=DEV)
        sR = slots * rows
        if ks:  # slot 0: the shared slice (member 0's rows for every member); slot 1: the member's own columns
            N.check(lib.amx_row_exponents(h, G, rows, ks, A.data_ptr(), ld, 0, rexp.data_ptr(), sR, 1, st),
                    "amx_row_exponents")
            N.check(lib.amx_row_exponents(h, G, rows, K - ks, A.data_ptr() + 4 * ks, ld, sA,
                                          rexp.data_ptr() + 4 * rows, sR, 1, st), "amx_row_exponents")
            slices = [inp["A"][:, :, :ks], inp["A"][:, :, ks:]]
        else:
            N.check(lib.amx_row_exponents(h, G, rows, K, A.data_ptr(), ld, sA, rexp.data_ptr(), sR, 1, st),
                    "amx_row_exponents")
            slices = [inp["A"]]
        got_exp = rexp.cpu().numpy()
        for i, sl in enumerate(slices):
            same(got_exp[:, i], X.row_exponent(sl).astype(np.int32), f"row exponents, slot {i}")
        assert (X.row_exponent(inp["A"])[:, inp["zero_row"]] == -100).all()
    elif c.path == "x6":
        W3 = torch.empty(G, Nw, 3 * K, dtype=torch.int16, device=DEV)
        N.check(lib.amx_split_bf16x3(h, G, Nw, K, Wd.data_ptr(), ld, sW, W3.data_ptr(), Nw * 3 * K, st),
                "amx_split_bf16x3")

    # ---- the output buffer, sentinels around the written slice
    if hidden:
        ldo, off, ncol = X.COL_OFF + Nw + X.LDC_PAD, X.COL_OFF, Nw
    else:
        ldo, off, ncol = c.S + X.LDP_PAD, 0, c.S
    out = torch.empty(G, rows, ldo, dtype=torch.float32, device=DEV)

    def launch():
        out.fill_(float(X.SENTINEL))
        if c.path == "h3" and hidden:
            rexp[:, in_slots].fill_(-100)
        o, sO, b = out.data_ptr(), rows * ldo, bias.data_ptr()
        if c.epi == "hidden_h3":
            rc = lib.amx_gemm_bias_act_h3(h, G, rows, Nw, K, A.data_ptr(), ld, sA, W2.data_ptr(), Nw * 2 * K,
                                          wexp.data_ptr(), Nw, b, Nw, o, ldo, sO, off, N.AMX_ACT_RELU,
                                          rexp.data_ptr(), sR, in_slots, rexp.data_ptr() + 4 * in_slots * rows, ks, st)
        elif c.epi == "out_h3":
            rc = lib.amx_gemm_out_unnorm_h3(h, G, rows, c.S, K, A.data_ptr(), ld, sA, W2.data_ptr(), Nw * 2 * K,
                                            wexp.data_ptr(), Nw, b, Nw, o, ldo, sO, rexp.data_ptr(), sR, in_slots,
                                            ks, st)
        elif c.epi == "hidden_x6":
            rc = lib.amx_gemm_bias_act_x6(h, G, rows, Nw, K, A.data_ptr(), ld, sA, W3.data_ptr(), Nw * 3 * K, b, Nw,
                                          o, ldo, sO, off, N.AMX_ACT_RELU, st)
        elif c.epi == "out_x6":
            rc = lib.amx_gemm_out_unnorm_x6(h, G, rows, c.S, K, A.data_ptr(), ld, sA, W3.data_ptr(), Nw * 3 * K, b,
                                            Nw, o, ldo, sO, st)
        elif c.epi == "out_f32":
            rc = lib.amx_gemm_out_unnorm(h, G, rows, c.S, K, A.data_ptr(), ld, sA, Wd.data_ptr(), ld, sW, b, Nw, o,
                                         ldo, sO, st)
        else:
            fn = lib.amx_gemm_bias_act_t64 if c.epi == "hidden_t64" else lib.amx_gemm_bias_act
            rc = fn(h, G, rows, Nw, K, A.data_ptr(), ld, sA, Wd.data_ptr(), ld, sW, b, Nw, o, ldo, sO, off,
                    N.AMX_ACT_RELU, st)
        N.check(rc, c.epi)
        torch.cuda.synchronize()
        return out.cpu().numpy(), (rexp[:, in_slots].cpu().numpy() if c.path == "h3" and hidden else None)

    # ---- the stream-K workspace of this case alone (NaN scratch: only written slots may be read)
    prior = getattr(ctx, "_split_ws", None)
    counters = None
    if c.ws:
        floats, ncnt = X.workspace_need(c.family, G, rows, Nw if hidden else 224, K)
        assert floats > 0 and ncnt > 0
        scratch = torch.full((floats,), float("nan"), dtype=torch.float32, device=DEV)
        counters = torch.zeros(ncnt, dtype=torch.int32, device=DEV)
        N.check(lib.amx_set_split_workspace(h, scratch.data_ptr(), floats, counters.data_ptr(), ncnt), "workspace")
    else:
        N.check(lib.amx_set_split_workspace(h, None, 0, None, 0), "workspace")
    try:
        got, got_exp_out = launch()
        if counters is not None:
            assert int(counters.abs().sum().item()) == 0, "stream-K arrival counters are not back at zero"
        again, again_exp = launch()
        if counters is not None:
            assert int(counters.abs().sum().item()) == 0
    finally:
        torch.cuda.synchronize()
        if prior is not None:
            lib.amx_set_split_workspace(h, prior[0].data_ptr(), prior[0].numel(), prior[1].data_ptr(), prior[1].numel())
        else:
            lib.amx_set_split_workspace(h, None, 0, None, 0)

    # ---- every element, the untouched surroundings, the zero row, the exponent output
    same(got[:, :, off:off + ncol], want, f"{c.family} output")
    assert (got[:, :, :off] == X.SENTINEL).all() and (got[:, :, off + ncol:] == X.SENTINEL).all(), \
        "columns outside the written slice were touched"
    zr = inp["zero_row"]
    b32 = inp["bias"].astype(np.float32)
    if hidden:
        zero_want = np.maximum(b32, np.float32(0))
    else:
        mu_d, sd_d = X.normalizers(c.S)[4:]
        zero_want = ((b32[:, :c.S] * sd_d[None, :]).astype(np.float32) + mu_d[None, :]).astype(np.float32)
    same(got[:, zr, off:off + ncol], zero_want, "zero row")
    if want_exp is not None and c.path == "h3":
        same(got_exp_out, want_exp.astype(np.int32), "row-exponent output")
        assert np.array_equal(again_exp, got_exp_out)
    assert got.tobytes() == again.tobytes(), "a second launch gave other bytes"
