"""What the mask patterns of tests/groups_cases.py reach, shown on the CPU with the float64 model alone: the conditions the GPU tests
(tests/test_gpu_groups.py) rely on hold on every shape, and every wrong model of a grouped match listed below gives another
answer than the right one on every shape with M >= 5 - so a kernel with that mistake cannot pass them.  One exception, asserted as
such: "the query mask of column fr taken from tile 0" is the right model where there is one query tile (M <= 32), and differs on
every shape with more."""
import numpy as np
import pytest

import groups_cases as gc
import match_cases as mc
import match_model as mm

SHAPES = mc.EXACT_SHAPES
MULTI = [s for s in SHAPES if s[1] >= 5]


def _right(S, rg, qg):
    Sm = gc.masked_scores(S, rg, qg)
    return mm.top1(Sm) + (mm.within(Sm, 0.0, 64)[2],)


def _case(N, M):
    S = gc.exact_scores(N, M)
    return S, gc.row_groups(N), gc.query_groups(M)


@pytest.mark.parametrize("N,M", SHAPES)
def test_patterns_meet_their_conditions(N, M):
    S, rg, qg = _case(N, M)
    P = gc.permitted(rg, qg)
    idx, cos, n0 = _right(S, rg, qg)
    pidx, pcos = mm.top1(S)
    pn0 = mm.within(S, 0.0, 64)[2]
    assert rg.dtype == qg.dtype == np.uint32 and rg.shape == (N,) and qg.shape == (M,)
    assert not np.any(rg & np.uint32(1 << 7)) and rg[N - 1] & np.uint32(1 << 6)
    if M == 1:
        # the negative query alone: it permits row N - 1 only, scores below -0.25 there; its second run permits nothing
        assert qg.tolist() == [1 << 6] and P[0].sum() == 1 and idx[0] == N - 1 and cos[0] < -0.25 and n0[0] == 0
        assert not gc.permitted(rg, gc.query_groups_none(1)).any()
        return
    assert qg[:4].tolist() == [1 << 2, 1 << 0, 0, 1 << 6]
    if N > gc.ANCHOR_COPY:
        # the anchor query: row 7 (the plain winner) is not permitted, its copy in the other half-wave, row 11, is
        assert pidx[mc.Q_ANCHOR] == mc.ANCHOR and not P[mc.Q_ANCHOR, mc.ANCHOR] and P[mc.Q_ANCHOR, gc.ANCHOR_COPY]
        assert idx[mc.Q_ANCHOR] == gc.ANCHOR_COPY and cos[mc.Q_ANCHOR] == 1.0
    # the negative query wins the last row of a ragged block with a score a masked element left at 0 would beat
    assert N % 32 != 0 and P[mc.Q_NEGATIVE].sum() == 1 and idx[mc.Q_NEGATIVE] == N - 1 and cos[mc.Q_NEGATIVE] < -0.25
    none, every = ~P.any(1), P.all(1)
    assert none[mc.Q_ZERO] and np.all(idx[none] == -1) and np.all(cos[none] == np.float32(-2.0)) and not n0[none].any()
    if M > 10:
        assert every[10] and idx[10] == pidx[10] and n0[10] == pn0[10]
    if M > 5:
        assert none[5]                                           # bit 7: no row has it
    assert int((idx != pidx).sum()) >= 5, int((idx != pidx).sum())
    assert int((n0 != pn0).sum()) >= 3


def _mutant(name, S, rg, qg):
    """top-1 and n_hits at min_cos = 0 of a wrong model of the grouped match"""
    M, N = S.shape
    P = gc.permitted(rg, qg)
    if name == "mask_ignored":
        return mm.top1(S) + (mm.within(S, 0.0, 64)[2],)
    if name == "host_post_filter":                               # unmasked selection, then the caller drops what is not permitted
        idx, cos = mm.top1(S)
        ok = (idx >= 0) & P[np.arange(M), np.maximum(idx, 0)]
        li, lc, ln = mm.within(S, 0.0, 64)
        kept = np.array([sum(1 for r in li[q] if r >= 0 and P[q, r]) for q in range(M)], np.int32)
        return np.where(ok, idx, -1).astype(np.int32), np.where(ok, cos, np.float32(-2.0)).astype(np.float32), kept
    if name == "query_mask_of_tile_0":                           # column fr of every tile takes the mask of query fr
        return _right(S, rg, qg[np.arange(M) % 32])
    if name.startswith("rows_shifted_"):                         # row r takes the mask of row r + s (past the table: 0)
        s = int(name.rsplit("_", 1)[1])
        sh = np.zeros(N, np.uint32)
        sh[:max(N - s, 0)] = rg[s:]
        return _right(S, sh, qg)
    if name == "masked_value_0":                                 # a row that is not permitted scores 0 instead of leaving the selection
        Z = np.where(P, S, np.float32(0.0)).astype(np.float32)
        return mm.top1(Z) + (mm.within(Z, 0.0, 64)[2],)
    if name == "rows_past_N_all":                                # the clamped copies of row N - 1 a ragged block reads count as members of every group
        pad = -N % 32
        Se = np.concatenate([S, np.repeat(S[:, N - 1:N], pad, axis=1)], axis=1)
        return _right(Se, np.concatenate([rg, np.full(pad, gc.ALL, np.uint32)]), qg)
    raise KeyError(name)


MUTANTS = ["mask_ignored", "host_post_filter", "query_mask_of_tile_0", "rows_shifted_4", "rows_shifted_8", "rows_shifted_32", "masked_value_0",
           "rows_past_N_all"]


@pytest.mark.parametrize("N,M", MULTI)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_models_give_another_answer(mutant, N, M):
    S, rg, qg = _case(N, M)
    want = _right(S, rg, qg)
    got = _mutant(mutant, S, rg, qg)
    same = all(mm.same_bits(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))
    if mutant == "query_mask_of_tile_0" and M <= 32:
        assert same                                              # (one query tile: tile 0 is the tile - the mistake needs M > 32 to show)
    else:
        assert not same, mutant
