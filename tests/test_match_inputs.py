"""Host tests (no device) of what tests/test_gpu_match_exact.py rests on: the exact family IS exact under fp32 arithmetic in any order,
fp32 arithmetic in several orders stays inside the derived bounds on the general and the normalisation family, the bounds that
replace the older tests' fitted tolerances are tighter than those on the tests' own inputs, and each of eight plausible kernel faults
(match_model.MUTANTS, run on a small numpy emulation) is rejected by at least one predicate the GPU file asserts."""
import numpy as np
import pytest

import match_cases as mc
import match_model as mm


# ---------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_rows_have_sum_of_squares_1024_and_planted_ties(N, M):
    G, Q = mc.exact_case(N, M)
    assert not G.flags.writeable and not Q.flags.writeable
    for rows in (G, Q):
        assert np.array_equal(rows, np.round(rows)) and np.abs(rows).max() <= 3
    assert np.all((G.astype(np.int64) ** 2).sum(1) == 1024)
    ssq = (Q.astype(np.int64) ** 2).sum(1)
    assert np.all((ssq == 1024) | (ssq == 0)) and (M == 1 or (ssq == 0).sum() == 1)
    planted = mc.planted_rows(N)
    if N > mc.ANCHOR + 32:
        assert {mc.ANCHOR + 4, mc.ANCHOR + 32, N // 2, N - 1} == set(planted) and len(planted) == 4
    elif N > mc.ANCHOR + 4:
        assert mc.ANCHOR + 4 in planted and N - 1 in planted
    for r in planted:
        assert np.array_equal(G[r], G[mc.ANCHOR])
    if M > 1 and N > mc.ANCHOR:
        assert np.array_equal(Q[mc.Q_ANCHOR], G[mc.ANCHOR]) and np.array_equal(Q[mc.Q_MINUS], -G[mc.ANCHOR])
        assert not Q[mc.Q_ZERO].any()


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_scores_are_exact_in_fp32_and_one_query_is_negative_everywhere(N, M):
    G, Q = mc.exact_case(N, M)
    g16, q16 = mc.unit16(G), mc.unit16(Q)
    assert np.array_equal(g16.astype(np.float64) * 32, G) and np.array_equal(q16.astype(np.float64) * 32, Q)
    absdot = np.abs(Q.astype(np.float64)) @ np.abs(G.astype(np.float64)).T          # = (|q| @ |g|.T) * 1024
    assert absdot.max() * 1024 < 2 ** 24                                             # any partial sum, in units of 2^-20: exact
    S = mm.scores(g16, q16)
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    assert np.array_equal(S * 1024, np.round(S * 1024))
    neg = 0 if M == 1 else mc.Q_NEGATIVE
    assert S[neg].max() < -0.25
    if M > 1 and N > mc.ANCHOR:
        hits = [mc.ANCHOR] + mc.planted_rows(N)
        assert np.all(S[mc.Q_ANCHOR, hits] == 1.0) and np.all(S[mc.Q_MINUS, hits] == -1.0)
        assert (S[mc.Q_ANCHOR] == 1.0).sum() == len(hits)
        assert not S[mc.Q_ZERO].any() and not np.signbit(S[mc.Q_ZERO]).any()


@pytest.mark.parametrize("N,M", [(129, 33), (257, 64)])
def test_exact_family_under_fp32_in_three_orders(N, M):
    G, Q = mc.exact_case(N, M)
    g16, q16 = mc.unit16(G), mc.unit16(Q)
    rng = np.random.default_rng(N)
    for order in ("kernel", "seq", "rand", "rand", "rand"):
        assert mm.same_bits(mm.normalize_fp32(G, order, rng), g16)
        assert mm.same_bits(mm.normalize_fp32(Q, order, rng), q16)
    want = mm.scores(g16, q16).astype(np.float32)
    for order in ("seq", "pair", "rand", "rand", "rand"):
        assert mm.same_bits(mm.scores_fp32(g16, q16, order, rng), want)


def test_identity_probe_and_identical_gallery():
    G16, Q16 = mc.identity_probe()
    assert np.array_equal(mm.scores(G16, Q16), G16.astype(np.float64).T)
    r, k = 299, 511
    assert float(G16[r, k]) == ((7 * r + 13 * k) % 127 - 63) / 64
    assert len(np.unique(G16.view(np.uint16))) == 127
    G, Q = mc.identical_case()
    S = mm.scores(mc.unit16(G), mc.unit16(Q))
    assert np.all(S[0] == 1.0) and np.all(S[1] == -1.0) and not S[2].any()
    idx, cos = mm.top1(S)
    assert idx.tolist() == [0, 0, 0] and cos.tolist() == [1.0, -1.0, 0.0]


def test_selections_on_a_hand_made_matrix():
    nan = np.nan
    S = np.array([[0.5, 1.0, 1.0, -1.0, nan],
                  [nan, nan, nan, nan, nan],
                  [-1.0, -1.0, nan, -1.0, -1.0]], np.float32)
    idx, cos = mm.top1(S)
    assert idx.tolist() == [1, -1, 0] and cos.tolist() == [1.0, -2.0, -1.0]
    idx, cos = mm.topk(S, 6)
    assert idx.tolist() == [[1, 2, 0, 3, -1, -1], [-1] * 6, [0, 1, 3, 4, -1, -1]]
    assert cos[0].tolist() == [1.0, 1.0, 0.5, -1.0, -2.0, -2.0]
    idx, cos, n = mm.within(S, 0.5, 2)
    assert n.tolist() == [3, 0, 0] and idx.tolist() == [[1, 2], [-1, -1], [-1, -1]]
    idx, cos, n = mm.within(S, -2.0, 3)
    assert n.tolist() == [4, 0, 4] and idx.tolist() == [[1, 2, 0], [-1, -1, -1], [0, 1, 3]]
    # the emulation without a mutant is the model
    assert all(mm.same_bits(a, b) for a, b in zip(mm.emulate_top1(S), mm.top1(S)))
    assert all(mm.same_bits(a, b) for a, b in zip(mm.emulate_within(S, 0.5, 2), mm.within(S, 0.5, 2)))


# ---------------------------------------------------------------------------------------------------- general family
def test_general_family_fp32_in_three_orders_stays_inside_the_bound():
    g16, q16 = mc.general_case(1000, 33)
    S, B = mm.scores(g16, q16), mm.score_bound(g16, q16)
    rng = np.random.default_rng(1)
    for order in ("seq", "pair", "rand"):
        got = mm.scores_fp32(g16, q16, order, rng)
        assert mm.scores_within_bound(got, g16, q16)
        print(f"fp32 {order}: largest err / bound {mm.worst_score(got, g16, q16):.4f}")
        ok, worst = mm.top1_within_bound(*mm.emulate_top1(got), S, B)
        assert ok, worst
    ordinary = np.setdiff1d(np.arange(33), np.arange(5, 10))
    b = B[ordinary]
    print(f"bound: median {np.median(b):.3e} max {b.max():.3e}")
    assert 2e-5 < np.median(b) < 6e-5 and b.max() < mm.D * mm.U23                   # unit rows: sum |q||g| <= 1
    assert (q16[5:9].view(np.uint16) & 0x7C00 == 0).any() and (g16[100:104].view(np.uint16) & 0x7C00 == 0).any()   # fp16 subnormals take part


def test_general_family_flushed_fp16_subnormals_exceed_the_bound():
    """the odd rows are there for this: a matrix unit that read fp16 subnormal operands as zero would miss the bound by orders of magnitude"""
    g16, q16 = mc.general_case(1000, 33)

    def flush(a):
        a = np.array(a)
        a[(a.view(np.uint16) & 0x7C00) == 0] = 0
        return a

    S, B = mm.scores(g16, q16), mm.score_bound(g16, q16)
    for g, q in ((flush(g16), q16), (g16, flush(q16))):
        assert (np.abs(mm.scores(g, q) - S) / B).max() > 100


def test_general_family_a_dropped_product_exceeds_the_bound():
    """condition of the GPU file's bound test: one dropped product is seen on >= 90 % of the (query, row) pairs, a dropped 16-wide
    k-step on >= 99 % (ordinary Gaussian rows and queries)"""
    g16, q16 = mc.general_case(1000, 33)
    ordinary = np.setdiff1d(np.arange(33), np.arange(5, 10))
    rows = np.setdiff1d(np.arange(1000), np.arange(100, 104))
    g, q = g16[rows].astype(np.float64), q16[ordinary].astype(np.float64)
    B = mm.score_bound(g16[rows], q16[ordinary])
    one = np.abs(q[:, 300, None] * g[None, :, 300])
    step = np.abs(q[:, 496:] @ g[:, 496:].T)
    s1, s16 = float((one > B).mean()), float((step > B).mean())
    print(f"seen: one product {100 * s1:.1f} %, one k-step {100 * s16:.1f} %")
    assert s1 >= 0.90 and s16 >= 0.99


# ---------------------------------------------------------------------------------------------------- normalisation
def test_normalisation_constant_is_the_documented_count():
    assert mm.C_NORM == 7.5 + 1 + 1 + 1 + 0.5 == 11 and mm.C_NORM <= 16
    assert "7.5" in mm.__doc__ and "C_NORM = 11" in mm.__doc__


def test_normalisation_family_fp32_in_three_orders_meets_the_bound():
    rows, kind = mc.normalization_rows()
    assert not rows.flags.writeable
    good = kind == mc.ORDINARY
    assert np.all(mm.in_domain(rows[good])) and not np.any(mm.in_domain(rows[(kind == mc.TOO_SMALL) | (kind == mc.TOO_LARGE)]))
    for k in (mc.ZERO, mc.TOO_SMALL, mc.TOO_LARGE, mc.HAS_NAN, mc.HAS_INF):
        i = int(np.nonzero(kind == k)[0][0])
        assert i % 4 == 2 and np.all(kind[[i - 2, i - 1, i + 1]] == mc.ORDINARY)      # among ordinary rows of its workgroup
    rng = np.random.default_rng(2)
    for order in ("kernel", "seq", "rand"):
        got = mm.normalize_fp32(rows, order, rng)
        ok, worst = mm.normalized_within_bound(got[good], rows[good])
        print(f"normalize fp32 {order}: largest err / bound {worst:.4f}")
        assert ok, worst
        for k in (mc.ZERO, mc.TOO_SMALL, mc.TOO_LARGE):
            assert not got[kind == k].astype(np.float32).any()
        for k in (mc.HAS_NAN, mc.HAS_INF):
            assert np.isnan(got[kind == k].astype(np.float32)).sum() == 1
    assert not mm.normalize(rows[kind == mc.ZERO]).any()


# ---------------------------------------------------------------------------------------------------- the bounds that replace fitted ones
@pytest.mark.parametrize("N,M", mc.PARITY_SHAPES)
def test_new_bound_is_below_the_old_1e_3_on_test_match_parity_inputs(N, M):
    G, Q = mc.parity_inputs(N, M)
    B = mm.public_score_bound(mm.to_f16(mm.normalize(G)), Q)
    print(f"match_parity {N} x {M}: largest bound {B.max():.3e}")
    assert B.max() < 1e-3
    assert mm.normalize_bound(G).max() < 1e-3


@pytest.mark.parametrize("N,M,k", mc.TOPK_SHAPES)
def test_new_bound_is_below_the_old_3e_3_on_test_match_topk_parity_inputs(N, M, k):
    G, Q = mc.topk_inputs(N, M, k)
    assert mm.public_score_bound(mm.to_f16(mm.normalize(G)), Q).max() < 3e-3


@pytest.mark.parametrize("N,M", mc.RUNNING_BEST_SHAPES)
def test_new_bound_is_below_the_old_1e_3_on_the_running_best_inputs(N, M):
    G, Q = mc.running_best_inputs(N, M)
    assert mm.public_score_bound(mm.to_f16(mm.normalize(G)), Q).max() < 1e-3


def test_new_bound_is_below_the_old_1e_3_on_the_snapshot_rows():
    assert mm.normalize_bound(mc.snapshot_rows()).max() < 1e-3


# ---------------------------------------------------------------------------------------------------- mutants
def _exact_small():
    G, Q = mc.exact_case(129, 33)
    g16, q16 = mc.unit16(G), mc.unit16(Q)
    return g16, q16, mm.scores(g16, q16).astype(np.float32)


def test_mutant_1_last_kstep_dropped():
    g16, q16, want = _exact_small()
    assert mm.same_bits(mm.emulate_scores(g16, q16), want)
    assert not mm.same_bits(mm.emulate_scores(g16, q16, "drop_last_kstep"), want)
    gg, gq = mc.general_case(1000, 33)
    assert mm.scores_within_bound(mm.emulate_scores(gg, gq), gg, gq)
    bad = mm.emulate_scores(gg, gq, "drop_last_kstep")
    assert not mm.scores_within_bound(bad, gg, gq)
    assert not mm.top1_within_bound(*mm.emulate_top1(bad), mm.scores(gg, gq), mm.score_bound(gg, gq))[0]


def test_mutant_2_query_chunks_swapped():
    g16, q16, want = _exact_small()
    assert not mm.same_bits(mm.emulate_scores(g16, q16, "swap_query_chunks"), want)
    G16, Q16 = mc.identity_probe()
    bad = mm.emulate_scores(G16[:40], Q16, "swap_query_chunks")
    assert not mm.same_bits(bad, G16[:40].astype(np.float32).T.copy())
    gg, gq = mc.general_case(1000, 33)
    assert not mm.scores_within_bound(mm.emulate_scores(gg, gq, "swap_query_chunks"), gg, gq)


def test_mutant_3_half_wave_rows_exchanged():
    g16, q16, want = _exact_small()
    bad = mm.emulate_scores(g16, q16, "swap_half_wave_rows")
    assert not mm.same_bits(bad, want)
    # the planted copy at 7 + 4 exists for this: top-1 of the anchor query moves from 7 to ... 3 (row 7's score lands on 3)
    assert mm.emulate_top1(bad)[0][mc.Q_ANCHOR] != mm.top1(want)[0][mc.Q_ANCHOR]
    G16, Q16 = mc.identity_probe()
    assert not mm.same_bits(mm.emulate_scores(G16[:40], Q16, "swap_half_wave_rows"), G16[:40].astype(np.float32).T.copy())


def test_mutant_4_ties_to_the_higher_row():
    _, _, want = _exact_small()
    good, bad = mm.emulate_top1(want), mm.emulate_top1(want, mutant="ties_to_higher_row")
    assert all(mm.same_bits(a, b) for a, b in zip(good, mm.top1(want)))
    assert bad[0][mc.Q_ANCHOR] == 128 and not mm.same_bits(bad[0], mm.top1(want)[0])


def test_mutant_5_rows_past_n_not_masked():
    g16, q16, want = _exact_small()
    N = 129
    padded = np.concatenate([want, np.repeat(want[:, N - 1:], 256 - N, axis=1)], axis=1)      # the clamped copies of row N - 1
    good = mm.emulate_within(padded, 1.0, 64, N_real=N)
    assert all(mm.same_bits(a, b) for a, b in zip(good, mm.within(want, 1.0, 64)))
    bad = mm.emulate_within(padded, 1.0, 64, N_real=N, mutant="unmasked_tail")
    assert bad[0].max() >= N and bad[2][mc.Q_ANCHOR] > good[2][mc.Q_ANCHOR]                    # reported at an index >= N
    assert not all(mm.same_bits(a, b) for a, b in zip(bad, mm.within(want, 1.0, 64)))


def test_mutant_6_strict_comparison_in_within():
    _, _, want = _exact_small()
    bound = float(want[mc.Q_NEGATIVE].max())                     # a value equal to one of the scores
    for min_cos in (1.0, bound):
        bad = mm.emulate_within(want, min_cos, 64, mutant="strict_within")
        assert not all(mm.same_bits(a, b) for a, b in zip(bad, mm.within(want, min_cos, 64)))


def test_mutant_7_truncating_fp16_conversion():
    rows, kind = mc.normalization_rows()
    good = kind == mc.ORDINARY
    assert mm.normalized_within_bound(mm.normalize_fp32(rows[good]), rows[good])[0]
    ok, worst = mm.normalized_within_bound(mm.normalize_fp32(rows[good], truncate=True), rows[good])
    assert not ok and worst > 1.5
    # (the exact family cannot see it: its unit rows are exact in fp16)
    G, _ = mc.exact_case(129, 33)
    assert mm.same_bits(mm.normalize_fp32(G, truncate=True), mc.unit16(G))


def test_mutant_8_minus_three_sentinel():
    _, _, want = _exact_small()
    S = want.copy()
    S[4] = np.nan                                                # what a NaN query scores
    idx, cos = mm.top1(S)
    assert idx[4] == -1 and cos[4] == np.float32(-2.0)
    assert all(mm.same_bits(a, b) for a, b in zip(mm.emulate_top1(S), (idx, cos)))
    bad = mm.emulate_top1(S, mutant="minus_three_sentinel")
    assert bad[0][4] == -1 and bad[1][4] == np.float32(-3.0) and not mm.same_bits(bad[1], cos)


def test_mutant_list_is_complete():
    import sys
    tests = [n for n in dir(sys.modules[__name__]) if n.startswith("test_mutant_") and n[12].isdigit()]
    assert len(tests) == len(mm.MUTANTS) == 8
