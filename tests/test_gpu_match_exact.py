"""GPU tests of the matcher (csrc/match.hip) and of normalize_rows_kernel against the float64 reference of tests/match_model.py.
Every expected value comes from match_model; none is read from the device.

exact family    integer rows of norm 32 (match_cases): every fp16 product and every fp32 partial sum in any order is exact, so scores,
                winners, lists and normalised rows equal the reference BIT FOR BIT - through the public entries (gallery_set / match /
                match_scores / match_within: normalize_rows_kernel is part of the chain) and through Engine.match_f16 (operands as
                fp16 bits; count on the host or in device memory).  The identity probe (one-hot queries) pins every fragment, swizzle
                and accumulator-row mapping element by element.
general family  unit Gaussian rows as fp16: |S_dev - scores()| <= score_bound elementwise; the persistent kernel's winner is within
                2 max(bound) of the best reference score and its cosine within the bound of its row's.  No query is left out.
normalisation   gallery_set + gallery_get within normalize_bound; zero and out-of-domain rows come back as zeros; NaN / inf rows leave
                their workgroup's other rows alone.
poison          NaN / +-65504 in reserved rows beyond the committed count, a NaN row inside the gallery, NaN / inf queries.
tests/test_match_inputs.py shows on the host that fp32 arithmetic meets these assertions on these inputs and that eight kernel faults do
not.  Largest err / bound measured on the device: DESIGN.md 4.11."""
import numpy as np
import pytest
import torch

import match_cases as mc
import match_model as mm
from frp_amd import dist as fdist
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

FILL_BITS = 0xFFFFFFFF
_REF = {}


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not mm.same_bits(got, want):
        view = np.uint32 if got.dtype == np.float32 else np.uint16 if got.dtype == np.float16 else got.dtype
        bad = np.argwhere(got.view(view) != want.view(view))
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _same_all(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{what}[{i}]")


def _exact_ref(N, M):
    """(G, Q, g16, q16, S float32) of one exact case: the reference, computed once and shared, never modified"""
    if (N, M) not in _REF:
        G, Q = mc.exact_case(N, M)
        g16, q16 = mc.unit16(G), mc.unit16(Q)
        S = mm.scores(g16, q16).astype(np.float32)
        S.setflags(write=False)
        _REF[(N, M)] = (G, Q, g16, q16, S)
    return _REF[(N, M)]


def _general_ref(N, M):
    if ("general", N, M) not in _REF:
        g16, q16 = mc.general_case(N, M)
        S, B = mm.scores(g16, q16), mm.score_bound(g16, q16)
        S.setflags(write=False)
        B.setflags(write=False)
        _REF[("general", N, M)] = (g16, q16, S, B)
    return _REF[("general", N, M)]


def _import_raw(engine, g16, capacity=None, tail=None):
    """the gallery as fp16 bits, not normalised: gallery_reserve, a torch copy, gallery_commit; `tail`: the reserved rows behind it"""
    N = g16.shape[0]
    cap = N if capacity is None else capacity
    ptr = engine.gallery_reserve(cap)
    t = torch.as_tensor(fdist._DevicePtr(ptr, cap, 512), device=torch.device("cuda", 0))
    t[:N].copy_(torch.from_numpy(np.array(g16)))
    if tail is not None:
        t[N:].copy_(torch.from_numpy(np.array(tail)))
    torch.cuda.synchronize()
    engine.gallery_commit(N)
    assert engine.gallery_size() == N


def _within_bounds(S):
    neg = 0 if S.shape[0] == 1 else mc.Q_NEGATIVE
    return [1.0, float(S[neg].max()), 0.0, -2.0]                # (the second one equals a score: `>=` is exercised)


# ------------------------------------------------------------------------------------------------ exact family, public entries
@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_public_scores_and_top1(engine, monkeypatch, N, M):
    G, Q, g16, q16, S = _exact_ref(N, M)
    engine.gallery_set(G)
    _same(engine.gallery_get(), g16, "gallery_get")
    _same(engine.match_scores(Q), S, "match_scores")
    want = mm.top1(S)
    _same_all(engine.match(Q), want, "match")                   # M <= 512: the persistent kernel
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    _same_all(engine.match(Q), want, "match, FRP_MATCH_V1")
    if M > 1 and N > mc.ANCHOR:
        assert want[0][mc.Q_ANCHOR] == mc.ANCHOR and want[1][mc.Q_ANCHOR] == 1.0 and S[mc.Q_MINUS, mc.ANCHOR] == -1.0


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_public_topk(engine, N, M):
    G, Q, _, _, S = _exact_ref(N, M)
    engine.gallery_set(G)
    idx, cos = mm.topk(S, 64)                                   # a prefix of the total order is the shorter list
    for k in (2, 7, 64):                                        # (k > N: the shapes with N = 1, 31, 33)
        _same_all(engine.match(Q, topk=k), (np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(cos[:, :k])), f"topk {k}")
    if N < 64:
        assert np.all(idx[:, N:] == -1) and np.all(cos[:, N:] == np.float32(-2.0))


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_public_within(engine, N, M):
    G, Q, _, _, S = _exact_ref(N, M)
    engine.gallery_set(G)
    for min_cos in _within_bounds(S):
        idx, cos, n = mm.within(S, min_cos, 64)
        if M > 1:                                               # the zero query scores exactly 0 on every row
            assert n[mc.Q_ZERO] == (N if min_cos <= 0 else 0)
        for cap in (64, 3):
            want = (np.ascontiguousarray(idx[:, :cap]), np.ascontiguousarray(cos[:, :cap]), n)
            _same_all(engine.match_within(Q, min_cos, cap), want, f"within {min_cos} cap {cap}")


def test_identical_rows(engine, monkeypatch):
    G, Q = mc.identical_case()
    S = mm.scores(mc.unit16(G), mc.unit16(Q)).astype(np.float32)
    engine.gallery_set(G)
    want = mm.top1(S)
    assert want[0].tolist() == [0, 0, 0] and want[1].tolist() == [1.0, -1.0, 0.0]
    _same(engine.match_scores(Q), S, "match_scores")
    _same_all(engine.match(Q), want, "match")
    _same_all(engine.match(Q, topk=7), mm.topk(S, 7), "topk")
    _same_all(engine.match_within(Q, -1.0, 64), mm.within(S, -1.0, 64), "within")
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    _same_all(engine.match(Q), want, "match, FRP_MATCH_V1")


# ------------------------------------------------------------------------------------------------ operands given as fp16
def test_identity_probe(engine, monkeypatch):
    G16, Q16 = mc.identity_probe()
    _import_raw(engine, G16)
    want_S = np.ascontiguousarray(G16.astype(np.float32).T) + np.float32(0.0)
    _same(want_S, mm.scores(G16, Q16).astype(np.float32), "the probe's reference")
    want = mm.top1(want_S)
    idx, cos, S = engine.match_f16(Q16, scores=True)
    _same(S, want_S, "S[k, r] == G[r, k]")
    _same_all((idx, cos), want, "per-tile kernel")
    _same_all(engine.match_f16(Q16), want, "persistent kernel")
    _same_all(engine.match_f16(Q16, n_device=512), want, "persistent kernel, device count")
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    _same_all(engine.match_f16(Q16), want, "FRP_MATCH_V1")


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_exact_f16_operands(engine, monkeypatch, N, M):
    _, _, g16, q16, S = _exact_ref(N, M)
    _import_raw(engine, g16)
    want = mm.top1(S)
    idx, cos, got = engine.match_f16(q16, scores=True)
    _same(got, S, "scores")
    _same_all((idx, cos), want, "per-tile kernel")
    _same_all(engine.match_f16(q16), want, "routed kernel")
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    _same_all(engine.match_f16(q16), want, "FRP_MATCH_V1")


@pytest.mark.parametrize("N,M", mc.GENERAL_SHAPES[:2])
def test_general_scores_within_bound(engine, N, M):
    g16, q16, S, B = _general_ref(N, M)
    _import_raw(engine, g16)
    idx, cos, got = engine.match_f16(q16, scores=True)
    err = np.abs(got.astype(np.float64) - S)
    odd_q = np.arange(5, 10)
    print(f"general {N} x {M}: largest err / bound {float((err / B).max()):.4f} (odd queries {float((err[odd_q] / B[odd_q]).max()):.4f}, "
          f"odd rows {float((err[:, 100:104] / B[:, 100:104]).max()):.4f})")
    assert np.all(err <= B), float((err / B).max())
    ok, worst = mm.top1_within_bound(idx, cos, S, B)
    assert ok, worst


@pytest.mark.parametrize("N,M", mc.GENERAL_SHAPES)
def test_general_top1_within_bound(engine, N, M):
    g16, q16, S, B = _general_ref(N, M)
    _import_raw(engine, g16)
    idx, cos = engine.match_f16(q16)                            # the persistent kernel: no score matrix
    ok, worst = mm.top1_within_bound(idx, cos, S, B)
    print(f"general top-1 {N} x {M}: largest |cos - r[i]| / b[i] {worst:.4f}, winners equal to the reference's "
          f"{int((idx == S.argmax(1)).sum())} of {M}")
    assert ok, worst


@pytest.mark.parametrize("N,M", [(257, 64), (70001, 512)])
def test_device_count(engine, N, M):
    _, _, g16, q16, S = _exact_ref(N, M)
    _import_raw(engine, g16)
    want = mm.top1(S)
    host = engine.match_f16(q16)
    _same_all(host, want, "host count")
    for n in (0, 1, 31, 32, 33, M):
        idx, cos = engine.match_f16(q16, n_device=n)
        _same_all((idx[:n], cos[:n]), (want[0][:n], want[1][:n]), f"device count {n}")
        assert np.all(idx[n:] == -1) and np.all(cos[n:].view(np.uint32) == FILL_BITS), n       # untouched: the 0xFF fill
        _same_all((idx[:n], cos[:n]), (host[0][:n], host[1][:n]), f"device count {n} against the host-count form")


def test_device_count_refusals(engine, monkeypatch):
    _, _, g16, q16, _ = _exact_ref(300, 513)
    _import_raw(engine, g16)
    with pytest.raises(FrpError):
        engine.match_f16(q16[:64], n_device=64, scores=True)    # the score matrix is the per-tile kernel's
    with pytest.raises(FrpError):
        engine.match_f16(q16, n_device=513)                     # more than FRP_MATCH_TOP1_MAX after rounding up to 32
    engine.match_f16(q16[:512], n_device=512)
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    with pytest.raises(FrpError):
        engine.match_f16(q16[:64], n_device=64)


# ------------------------------------------------------------------------------------------------ normalisation
def test_normalisation_family(engine):
    rows, kind = mc.normalization_rows()
    engine.gallery_set(rows)
    got = engine.gallery_get()
    good = kind == mc.ORDINARY
    ok, worst = mm.normalized_within_bound(got[good], rows[good])
    print(f"normalisation: largest err / bound {worst:.4f}")
    assert ok, worst
    for k in (mc.ZERO, mc.TOO_SMALL, mc.TOO_LARGE):
        assert not got[kind == k].astype(np.float32).any(), k   # zero rows (of either sign of zero)
    clean = np.array(rows)
    clean[(kind == mc.HAS_NAN) | (kind == mc.HAS_INF)] = 0
    engine.gallery_set(clean)
    _same(engine.gallery_get()[good], got[good], "rows next to the NaN and inf rows")
    engine.gallery_set(rows.astype(np.float64))                 # fp64 host rows: the fp32 rows widened -> the same bytes
    again = engine.gallery_get()
    assert again[good].tobytes() == got[good].tobytes()


# ------------------------------------------------------------------------------------------------ poison
def _public_results(engine, Q, monkeypatch):
    out = {"scores": engine.match_scores(Q), "match": engine.match(Q), "topk": engine.match(Q, topk=7),
           "within 1": engine.match_within(Q, 1.0, 64), "within -2": engine.match_within(Q, -2.0, 3)}
    with monkeypatch.context() as m:
        m.setenv("FRP_MATCH_V1", "1")
        out["match v1"] = engine.match(Q)
    return out


def _public_reference(S):
    return {"scores": S, "match": mm.top1(S), "topk": mm.topk(S, 7), "within 1": mm.within(S, 1.0, 64),
            "within -2": mm.within(S, -2.0, 3), "match v1": mm.top1(S)}


def _compare_results(got, want, nan_rows=(), nan_cols=()):
    """bit for bit; the score matrix's NaN rows / columns are compared as NaN (a payload is not part of the contract)"""
    S, W = np.array(got["scores"]), np.array(want["scores"])
    for sl in [np.s_[list(nan_rows), :], np.s_[:, list(nan_cols)]]:
        assert np.all(np.isnan(S[sl])) and np.all(np.isnan(W[sl]))
        S[sl], W[sl] = 0, 0
    _same(S, W, "scores")
    for name in want:
        if name != "scores":
            _same_all(got[name], want[name], name)


@pytest.mark.parametrize("N", [129, 1000])
def test_poison_behind_the_committed_rows(engine, monkeypatch, N):
    """300 reserved rows beyond the committed count hold NaN bits and +-65504: nothing beyond N may be read and then masked by
    arithmetic (0 * NaN, a clamp that lands on them): every result equals the reference of the N rows"""
    _, Q, g16, _, S = _exact_ref(N, 33)
    tail = np.empty((300, 512), np.float16)
    tail[0::3] = np.float16(np.nan)
    tail[1::3] = np.float16(65504.0)
    tail[2::3] = np.float16(-65504.0)
    tail[5].view(np.uint16)[:] = 0xFFFF
    _import_raw(engine, g16, capacity=N + 300, tail=tail)
    _compare_results(_public_results(engine, Q, monkeypatch), _public_reference(S))


def test_poison_nan_row_in_the_gallery(engine, monkeypatch):
    """row 7 + 4 (a planted copy of the anchor: without the NaN it would be second in the anchor query's lists) is NaN: every other
    row's scores are unchanged, the row is never a winner, never in a top-k list, never a within hit"""
    N, M = 129, 33
    _, Q, g16, q16, S0 = _exact_ref(N, M)
    bad = mc.ANCHOR + 4
    g = np.array(g16)
    g[bad] = np.float16(np.nan)
    S = mm.scores(g, q16).astype(np.float32)
    assert np.all(np.isnan(S[:, bad])) and np.array_equal(np.delete(S, bad, 1), np.delete(S0, bad, 1))
    want = _public_reference(S)
    assert not any(np.any(want[k][0] == bad) for k in want if k != "scores")
    _import_raw(engine, g)
    _compare_results(_public_results(engine, Q, monkeypatch), want, nan_cols=[bad])
    idx, cos, got = engine.match_f16(q16, scores=True)
    _compare_results({"scores": got, "match": (idx, cos)}, {"scores": S, "match": want["match"]}, nan_cols=[bad])
    _same_all(engine.match_f16(q16), want["match"], "persistent kernel")


def test_poison_nan_and_inf_queries(engine, monkeypatch):
    """a NaN query and an inf query among ordinary queries of the same 32-query tile: the ordinary queries' results are unchanged, the
    poisoned ones get -1 / -2.0 from match (both kernels), match(topk) and match_within (n_hits 0)"""
    N, M = 129, 33
    G, Q0, g16, _, S0 = _exact_ref(N, M)
    Q = np.array(Q0)
    Q[10, 5] = np.nan
    Q[20, 9] = np.inf
    S = mm.scores(g16, mm.to_f16(mm.normalize(Q))).astype(np.float32)
    assert np.all(np.isnan(S[[10, 20]])) and np.array_equal(np.delete(S, [10, 20], 0), np.delete(S0, [10, 20], 0))
    want = _public_reference(S)
    for name in ("match", "match v1", "topk", "within 1", "within -2"):
        assert np.all(want[name][0][[10, 20]] == -1) and np.all(want[name][1][[10, 20]] == np.float32(-2.0))
    assert want["within -2"][2][[10, 20]].tolist() == [0, 0] and want["within -2"][2][0] == N
    engine.gallery_set(G)
    _compare_results(_public_results(engine, Q, monkeypatch), want, nan_rows=[10, 20])
