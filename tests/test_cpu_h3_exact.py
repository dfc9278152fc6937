"""The exactly summable operands of tests/h3_exact.py and its case table, checked without a GPU:
the limbs are the ones the builders intend, the exactness condition holds for every case, the
table reaches every tile family it names (pick_tile at 256 CUs), and the numpy restatement of
the f16x3 algorithm relates to a plain fp64 A W^T as it should."""
import numpy as np
import pytest

import h3_exact as X

H3_FAMILIES = {"H256", "HRow<4>", "HRow<5>", "HRow<6>", "HRow<7>", "HS64", "HS64w8", "H128k32", "H128",
               "H128x224", "H128x224 stream-K", "H80x224", "H128x224k16",
               "HOut<4,7>", "HOut<6,7>", "HOut<7,7>", "HOut<4,8>", "HOut<5,8>", "HOut<6,8>", "HOut<7,8>",
               "H128x256", "HS32", "HS32w8"}
OTHER_FAMILIES = {"X256", "X128", "X128x224", "T128", "T128x224", "k_gemm64_fwd"}


def test_table_reaches_every_family():
    """pick_tile of each case is the family written beside it, every family of the launchers is
    in the table in both tiers (the bf16x6 / f32 tiles in tier 1), the 2304-deep K stays with the
    stream-K families, and each stream-K family has a K at which its tiles split."""
    for c in X.CASES:
        assert X.pick_tile(X.N_CUS, c.epi, c.groups, c.rows, c.N, c.K, c.S, c.ws) == c.family, c
        assert (c.K == 2304) <= (c.family in X.STREAM_K), c
        assert c.k_shared % 32 == 0 and c.k_shared < c.K
    for tier in (1, 2):
        assert {c.family for c in X.CASES if c.path == "h3" and c.tier == tier} == H3_FAMILIES
    assert {c.family for c in X.CASES if c.path != "h3"} == OTHER_FAMILIES
    assert all(c.tier == 1 for c in X.CASES if c.path != "h3")
    # S = 100 and S = 300 reach the 128 x 128 output tiles; both BK-16 output shapes are there
    assert {(c.family, c.S) for c in X.CASES if c.epi == "out_h3" and c.S in (100, 300)} == \
        {("H128k32", 100), ("H128k32", 300), ("H128", 100), ("H128", 300)}
    for fam in ("HS64", "HS64w8", "HS32", "HS32w8"):
        splits = {X.small_plan(c.groups, c.rows, 512 if fam.startswith("HS64") else 224, c.K, X.TILE[fam][1])[2]
                  for c in X.CASES if c.family == fam}
        assert splits == {1, 2, 8}, (fam, splits)
    # without the workspace the stream-K shapes fall to the tiles the table lists for them
    assert X.pick_tile(256, "out_h3", 4, 4096, 256, 352, 197, False) == "HOut<4,7>"
    assert X.pick_tile(256, "hidden_h3", 4, 256, 512, 352, 197, False) == "H128k32"
    # a workspace need is stated exactly for the families that use one
    for c in X.CASES:
        assert (X.workspace_need(c.family, c.groups, c.rows, 512 if c.epi == "hidden_h3" else 224, c.K)[0] > 0) \
            == (c.family in X.STREAM_K)


def test_limb_identities():
    """tier 1: lo = 0 and hi 2^(E-14) is the operand; tier 2: in scaled units hi = 1024 p or the
    anchor 8192, lo = +-1/4 (0 under the anchor and the zeros), neither conversion a tie, E the
    anchor's exponent; both reconstruct exactly.  A tier-2 W row has its nonzeros at
    tier2_w_positions and the anchor, and the rows of a 64-column tile together touch every k at
    K <= 352 (of a 224-column tile at K = 2304; the 32- and 64-column stream-K tiles have too few
    nonzeros for that -- 89 % of k at 32 columns and K = 352, a third at 64 columns and K = 2304
    -- and lean on the dense tier 1 there)."""
    rs = np.random.RandomState(0)
    for K in (32, 48, 96, 352, 2304):
        a1, a2, w2 = X.tier1(rs, (2, 64, K)), X.tier2_a(rs, (2, 64, K)), X.tier2_w(rs, (2, 256, K))
        for x in (a1, a2, w2):
            assert x.dtype == np.float32
            E = X.row_exponent(x)
            hi, lo = X.split_limbs(x, E)
            assert np.array_equal(np.ldexp(hi + lo, (E - X.HSC)[..., None]), x.astype(np.float64))
            ref = (np.abs(hi).max(-1), np.abs(lo).max(-1), np.abs(hi).sum(-1), np.abs(lo).sum(-1),
                   X.granule(hi), X.granule(lo))
            assert all(np.array_equal(u, v) for u, v in zip(X.row_stats(x[0]), [r[0] for r in ref]))
        assert (np.abs(a1) > 0).any(-1).all()
        hi, lo = X.split_limbs(a1, X.row_exponent(a1))
        assert not lo.any()
        ints = a1.astype(np.float64) / X.granule(a1)[..., None]  # over the row's granule: integers
        assert np.array_equal(ints, np.rint(ints)) and np.abs(ints).max() <= 15
        for x, dense in ((a2, True), (w2, False)):
            E = X.row_exponent(x)
            xs = np.ldexp(x.astype(np.float64), (X.HSC - E)[..., None])
            hi, lo = X.split_limbs(x, E)
            assert (np.abs(xs).max(-1) == 8192).all() and ((xs == 8192).sum(-1) == 1).all()
            body = (xs != 8192) & (xs != 0)
            assert body[xs != 8192].all() if dense else True
            assert np.isin(np.abs(hi[body]), 1024.0 * np.arange(1, 8)).all() and (np.abs(lo[body]) == 0.25).all()
            assert (np.abs(np.abs(xs[body]) - 1023.75) > 0).all()  # the one tie of the value set
            assert not lo[~body].any()
            # not a tie: the fp16 neighbours of xs are hi and hi +- ulp, |xs - hi| = 1/4 < ulp / 2 (ulp >= 1)
            assert (np.abs(xs - hi) <= 0.25).all() and (np.spacing(np.abs(hi[body]).astype(np.float16)) >= 1).all()
        nz = w2[0] != 0
        for n in (0, 1, 100, 255):
            want = np.zeros(K, bool)
            want[X.tier2_w_positions(n, K)] = True
            extra = nz[n] & ~want
            assert (nz[n] | ~want).all() and extra.sum() <= 1
        bn = 64 if K <= 352 else 224
        for c0 in range(0, 256 - bn + 1, bn):
            assert nz[c0:c0 + bn].any(0).all()


@pytest.mark.parametrize("tier,K", sorted({(c.tier, c.K) for c in X.CASES}))
def test_exactness_condition_every_case(tier, K):
    """sum_k |hi||hi'| + |hi||lo'| + |lo||hi'| < 2^22 granules for every output of every case (a
    condition on the inputs, not a tolerance on the kernel), through the bound from row maxima
    and row sums, which is at least the sum itself.  On the small cases the inputs are built
    whole: the sum itself (three matrix products) lies under the bound, the NaN columns, the
    shared leading columns and the zero row are where case_inputs says."""
    for c in [c for c in X.CASES if (c.tier, c.K) == (tier, K)]:
        bound = X.case_bound(c)
        assert 0 < bound < 2.0 ** 22, (c, np.log2(bound))
        if c.rows > 256:
            continue
        inp = X.case_inputs(c)
        assert inp["A"].shape == (c.groups, c.rows, c.K) and inp["W"].shape == (c.groups, c.N, c.K)
        assert np.isnan(inp["A_dev"][:, :, c.K:]).all() and np.isnan(inp["W_dev"][:, :, c.K:]).all()
        assert not inp["A"][:, inp["zero_row"]].any() and np.isfinite(inp["A"]).all()
        if c.k_shared:
            assert np.isnan(inp["A_dev"][1:, :, :c.k_shared]).all()
            assert np.array_equal(inp["A_dev"][0, :, :c.K], inp["A"][0])
            assert np.array_equal(inp["A_dev"][1:, :, c.k_shared:c.K], inp["A"][1:, :, c.k_shared:])
            assert np.array_equal(inp["A"][1:, :, :c.k_shared], np.broadcast_to(
                inp["A"][0, :, :c.k_shared], inp["A"][1:, :, :c.k_shared].shape))
        else:
            assert np.array_equal(inp["A_dev"][:, :, :c.K], inp["A"])
        for g in range(c.groups):
            exact = X.exactness_max(inp["A"][g], inp["W"][g])
            assert 0 < exact <= X.exactness_bound(inp["A"][g], inp["W"][g]) <= bound
            # the rows' scales differ (at least 20 of the 41 exponents occur)
            assert len(np.unique(X.row_exponent(inp["W"][g]))) >= 20
            assert len(np.unique(X.row_exponent(inp["A"][g]))) >= 20


def test_restatement_against_fp64():
    """On tier 1 the three-product value, un-scaled, is A W^T exactly; on tier 2 it misses it by
    exactly the dropped sum of lo lo'."""
    rs = np.random.RandomState(1)
    for K in (32, 352, 2304):
        for tier in (1, 2):
            A = (X.tier1 if tier == 1 else X.tier2_a)(rs, (1, 96, K))[0]
            W = (X.tier1 if tier == 1 else X.tier2_w)(rs, (1, 128, K))[0]
            A[5] = 0.0
            acc, Er, Ec = X.h3_acc(A, W)
            sh = Er[:, None] + Ec[None, :] - 2 * X.HSC
            full = A.astype(np.float64) @ W.astype(np.float64).T
            al, wl = X.split_limbs(A, Er)[1], X.split_limbs(W, Ec)[1]
            dropped = np.ldexp(al @ wl.T, sh)
            assert np.array_equal(full - np.ldexp(acc, sh), dropped)
            assert dropped.any() == (tier == 2)
            assert np.array_equal(X.pre_bias(A, W, "h3").astype(np.float64), np.ldexp(acc, sh))
            assert Er[5] == -100 and not np.ldexp(acc, sh)[5].any()
            if tier == 1:
                assert np.array_equal(X.pre_bias(A, W, "f32"), X.pre_bias(A, W, "h3"))


def test_epilogues_round_per_operation():
    """The restated epilogues round once per fp32 operation, keep -0 / +0 as values and give the
    bias alone on a zero row."""
    pre = np.array([[0.0, 3.0, -5.0, 2.0 ** 24]], np.float32)
    bias = np.array([-1.0, 0.5, 1.0, 1.0], np.float32)
    v, e = X.hidden_epilogue(pre, bias)
    assert np.array_equal(v, np.array([[0.0, 3.5, 0.0, 2.0 ** 24]], np.float32)) and e.tolist() == [25]
    assert X.hidden_epilogue(np.zeros((1, 4), np.float32), -np.abs(bias))[1].tolist() == [-100]
    sd, mu = np.array([3.0, 1.0 / 3.0, 1.5, 1.0], np.float32), np.array([1.0, 1e-3, 0.0, 0.5], np.float32)
    got = X.output_epilogue(pre, bias, sd, mu)
    y = pre[0] + bias
    want = [np.float32(np.float32(y[i] * sd[i]) + mu[i]) for i in range(4)]
    assert np.array_equal(got[0], np.array(want, np.float32))
