"""GPU tests of the radius match (frp_match_within, FRP_FLAG_WITHIN / frp_fetch_within, FaceService on top of them): the rows of
the gallery whose cosine with a query is at or above a bound, listed by the match kernels' own epilogue.  The expected lists come
from the device's score matrix (Engine.match_scores: the per-tile kernel's all_scores epilogue, which this feature leaves alone):
stable argsort by descending score cut at the bound, cosines bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.face_service import WITHIN_CAP, FaceService
from frp_amd.native import FrpError
from oracle import network as onet

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(1, 1), (31, 5), (1000, 33), (4097, 320), (70001, 512), (300, 513)]


def _expected(S, min_cos, cap):
    """lists from a score matrix: (idx [M, cap], cos [M, cap], n [M])"""
    M = S.shape[0]
    idx = np.full((M, cap), -1, np.int32)
    cos = np.full((M, cap), -2.0, np.float32)
    n = np.zeros(M, np.int32)
    for q in range(M):
        order = np.argsort(-S[q].astype(np.float64), kind="stable")
        order = order[S[q, order] >= np.float32(min_cos)]
        n[q] = len(order)
        k = min(len(order), cap)
        idx[q, :k] = order[:k]
        cos[q, :k] = S[q, order[:k]]
    return idx, cos, n


def _same_lists(got, want):
    for g, w, what in zip(got, want, ("idx", "cos", "n_hits")):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32)) if g.dtype == np.float32 else np.argwhere(g != w)
        assert len(bad) == 0, (what, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


_EDGE = {}


def _edge_case(engine, N, M):
    """gallery, queries and the device's score matrix of one shape (computed once, shared, never modified); leaves the gallery set"""
    if (N, M) not in _EDGE:
        rng = np.random.default_rng(N * 1000 + M + 17)
        G = rng.standard_normal((N, 512)).astype(np.float32)
        G /= np.linalg.norm(G, axis=1, keepdims=True)
        if N > 64:
            G[N - 1] = G[7]                     # duplicates far apart: other waves, other workgroups; the tie order is visible
            G[N // 2] = G[7]
        Q = G[rng.integers(0, N, size=M)] + 0.5 * rng.standard_normal((M, 512)).astype(np.float32) / np.sqrt(512)
        if N > 64:
            Q[0] = G[7]
        engine.gallery_set(G)
        S = engine.match_scores(Q)
        S.setflags(write=False)
        _EDGE[(N, M)] = (G, Q, S)
    G, Q, S = _EDGE[(N, M)]
    engine.gallery_set(G)
    return G, Q, S


@pytest.mark.parametrize("N,M", EDGE_SHAPES)
def test_match_within_tile_and_block_edges(engine, N, M):
    """a gallery smaller than a block, ragged last blocks, 1 / 2 / 16 query tiles, 513 queries (the per-tile kernel); the bound
    EQUALS a score (the 5th largest of query 0), so `>=` is exercised, and the planted duplicates tie across workgroups"""
    G, Q, S = _edge_case(engine, N, M)
    min_cos = float(np.sort(S[0])[::-1][min(4, N - 1)])
    for cap in (64, 3):
        got = engine.match_within(Q, min_cos, cap)
        want = _expected(S, min_cos, cap)
        if cap == 3:        # lists that overflow come from the score rows: the same order, the true count
            assert want[2].max() > 3 or N < 5
        _same_lists(got, want)
    idx, cos, n = engine.match_within(Q, min_cos, 64)
    assert n[0] >= min(5, N)
    if N > 64:
        assert idx[0, :3].tolist() == [7, N // 2, N - 1] and cos[0, 0] == cos[0, 1] == cos[0, 2]
    i1, c1 = engine.match(Q)                          # the top-1 of the same kernels heads every non-empty list
    assert np.array_equal(idx[n > 0, 0], i1[n > 0]) and np.array_equal(cos[n > 0, 0], c1[n > 0])


@pytest.mark.parametrize("min_cos", [-2.0, 0.0])
def test_match_within_padding_emits_nothing(engine, min_cos):
    """M = 5 of a 32-query tile, N = 40 of a 128-row block: the 27 zero query rows score exactly 0 >= min_cos and the rows past
    N are clamped copies of row 39 - neither may be listed.  All scores of these queries are positive, so both bounds list all 40."""
    rng = np.random.default_rng(40)
    base = rng.standard_normal(512).astype(np.float32)
    G = base[None] + 0.7 * rng.standard_normal((40, 512)).astype(np.float32)
    Q = base[None] + 0.7 * rng.standard_normal((5, 512)).astype(np.float32)
    engine.gallery_set(G)
    S = engine.match_scores(Q)
    assert S.min() > 0.2                                # the seeded data: every row is a hit for either bound
    idx, cos, n = engine.match_within(Q, min_cos, 64)
    assert n.tolist() == [40] * 5
    _same_lists((idx, cos, n), _expected(S, min_cos, 64))
    assert np.array_equal(np.sort(idx[:, :40], axis=1), np.tile(np.arange(40, dtype=np.int32), (5, 1)))
    assert np.all(idx[:, 40:] == -1) and np.all(cos[:, 40:] == -2.0)


def test_match_within_cap_edges_and_determinism(engine):
    """66 copies of one row spread over 3000: a query with exactly 64 hits, one with 66 (true count, the 64 lowest rows in order:
    which 64 took the slots in the kernel is a race, the list is rebuilt from the score row), one with none; twice, bit-equal"""
    rng = np.random.default_rng(66)
    N = 3000
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    dup = np.sort(rng.choice(N, size=66, replace=False))
    v = G[dup[0]].copy()
    G[dup] = v
    # a second family of 66 copies whose last two are perturbed away: exactly 64 hits for its query
    dup2 = np.sort(rng.choice(np.setdiff1d(np.arange(N), dup), size=66, replace=False))
    w = G[dup2[0]].copy()
    G[dup2] = w
    far = w + 0.6 * rng.standard_normal(512).astype(np.float32) / np.sqrt(512)
    G[dup2[-2:]] = far / np.linalg.norm(far)
    none = rng.standard_normal(512).astype(np.float32)
    Q = np.stack([w, v, none])
    engine.gallery_set(G)
    S = engine.match_scores(Q)
    s_far, s_copy = float(S[0, dup2[-1]]), float(S[0, dup2[0]])
    assert s_far < 0.95 < s_copy and float(np.sort(S[0])[::-1][66]) < 0.5          # the bound lies between
    min_cos = 0.95
    assert S[2].max() < min_cos
    a = engine.match_within(Q, min_cos, 64)
    b = engine.match_within(Q, min_cos, 64)
    _same_lists(a, b)
    _same_lists(a, _expected(S, min_cos, 64))
    idx, cos, n = a
    assert n.tolist() == [64, 66, 0]
    assert idx[0].tolist() == dup2[:64].tolist() and idx[1].tolist() == dup[:64].tolist()
    assert np.all(idx[2] == -1) and np.all(cos[2] == -2.0)


def test_match_within_no_stale_state(engine):
    """hit counters and lists start from zero in every pass: many hits, then none, on the same handle"""
    rng = np.random.default_rng(8)
    G = rng.standard_normal((500, 512)).astype(np.float32)
    Q = rng.standard_normal((40, 512)).astype(np.float32)
    engine.gallery_set(G)
    idx, cos, n = engine.match_within(Q, -2.0, 64)
    assert n.tolist() == [500] * 40 and np.all(idx >= 0)
    idx, cos, n = engine.match_within(Q, 0.9, 64)
    assert not n.any() and np.all(idx == -1) and np.all(cos == -2.0)


def test_match_within_errors(engine):
    q = np.ones((1, 512), np.float32)
    engine.gallery_set(np.eye(4, 512, dtype=np.float32))
    for cap in (0, 65):
        with pytest.raises(FrpError):
            engine.match_within(q, 0.5, cap)
    with pytest.raises(FrpError):
        engine.match_within(q, float("nan"), 8)
    idx, cos = np.empty((1, 8), np.int32), np.empty((1, 8), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine._lib.frp_match_within(engine._h, ptr(q), 1, 0.5, 8, ptr(idx), ptr(cos), None)
    assert rc == -1
    with pytest.raises(FrpError):
        engine._chk(rc)
    engine.gallery_set(np.zeros((0, 512), np.float32))
    with pytest.raises(FrpError, match="gallery is empty"):
        engine.match_within(q, 0.5, 8)


def test_match_within_against_the_fp64_oracle(engine):
    """independent of the device's scores: membership against oracle.network.match_topk on the fp32 operands, asserted for the
    rows whose fp64 cosine lies more than 3e-3 (test_match_topk_parity's cosine tolerance) from the bound"""
    N, M = 1000, 33
    G, Q, S = _edge_case(engine, N, M)
    Qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    oidx, ocos = onet.match_topk(G, Qn, N)                       # every row, ordered: [M, N]
    ref = np.empty((M, N))
    np.put_along_axis(ref, oidx.astype(np.int64), np.asarray(ocos, dtype=np.float64), axis=1)
    min_cos, tol = 0.12, 3e-3
    clear_hit, clear_miss = ref > min_cos + tol, ref < min_cos - tol
    assert np.all(clear_hit.sum(1) >= 1) and np.all(clear_miss.sum(1) >= 1)       # the reference alone: the data decides something
    assert np.all(clear_hit.sum(1) <= 64)
    idx, cos, n = engine.match_within(Q, min_cos, 64)
    for q in range(M):
        got = set(idx[q, :min(n[q], 64)].tolist())
        assert set(np.nonzero(clear_hit[q])[0].tolist()) <= got
        assert not (set(np.nonzero(clear_miss[q])[0].tolist()) & got)
        k = min(n[q], 64)
        assert np.abs(cos[q, :k] - ref[q, idx[q, :k]]).max() < tol


def _frames(rng, B, H, W):
    base = rng.integers(0, 255, size=(B, H // 16, W // 16, 3)).astype(np.float32)
    base = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    return np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)


def _planted(engine, rng, frames, K):
    """embeddings of the engine's own faces (forced-K: slot 0 of a frame is its best anchor, also what threshold mode keeps first)
    planted into a gallery: face (0, 0) twice - an exact tie - plus a near copy, face (1, 0) once"""
    engine.gallery_set(np.zeros((0, 512), np.float32))
    e = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_NO_MATCH)["emb"]
    G = rng.standard_normal((700, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    G[400] = G[10] = e[0, 0]
    G[650] = e[0, 0] + 0.1 * rng.standard_normal(512).astype(np.float32) / np.sqrt(512)
    G[5] = e[1, 0]
    return G


@pytest.mark.selfcheck
def test_fused_within_pass_equals_plain_pass_and_match_within(fresh_engine):
    """FRP_FLAG_WITHIN changes nothing else about a pass (top-1, cosine, embeddings bit for bit) and its lists are those of
    match_within on the fetched embeddings; threshold mode keeps the face count on the device, forced-K knows it on the host"""
    engine = fresh_engine
    rng = np.random.default_rng(2024)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 6
    frames = _frames(rng, B, H, W)
    G = _planted(engine, rng, frames, K)
    engine.gallery_set(G)
    probe = engine.detect(frames, max_faces=K, det_thresh=1e-6)
    sc = np.sort(probe["scores"][0, :probe["counts"][0]])[::-1]
    assert len(sc) >= 3
    thr = float(0.5 * (sc[1] + sc[2]))                   # frame 0 keeps two faces: empty slots, a count below the capacity
    min_cos, cap = 0.9, 8
    engine.set_within(min_cos, cap)
    with pytest.raises(FrpError):
        engine.fetch_within()                            # nothing flagged yet
    for flags, dt in ((0, thr), (native.FLAG_FORCED_K, 0.5)):
        a = engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags)
        b = engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags | native.FLAG_WITHIN)
        for k in ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        idx, cos, n = engine.fetch_within()
        assert idx.shape == (B, K, cap) and n.shape == (B, K)
        live = np.arange(K)[None, :] < b["counts"][:, None]
        assert live.any() and (flags or not live.all())
        assert not n[~live].any() and np.all(idx[~live] == -1) and np.all(cos[~live] == -2.0)
        w = engine.match_within(b["emb"][live], min_cos, cap)
        _same_lists((idx[live], cos[live], n[live]), w)
        assert n.max() <= cap                            # (no list of this part overflows)
        assert n[0, 0] >= 3 and idx[0, 0, :2].tolist() == [10, 400] and cos[0, 0, 0] == cos[0, 0, 1] and 650 in idx[0, 0]
        assert idx[1, 0, 0] == 5
        assert np.array_equal(idx[live][n[live] > 0, 0], b["match_idx"][live][n[live] > 0])
        assert np.array_equal(cos[live][n[live] > 0, 0], b["match_cos"][live][n[live] > 0])
        idx2, cos2, n2 = engine.fetch_within()           # a second fetch: the same
        _same_lists((idx2, cos2, n2), (idx, cos, n))
        with pytest.raises(FrpError):                    # a pass without the flag has no lists
            engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags)
            engine.fetch_within()
    # a list that overflows is rebuilt at fetch time from the embeddings the pass left on the device
    engine.set_within(min_cos, 2)
    b = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_WITHIN)
    idx, cos, n = engine.fetch_within()
    assert n[0, 0] >= 3 and idx[0, 0].tolist() == [10, 400]
    _same_lists((idx.reshape(-1, 2), cos.reshape(-1, 2), n.reshape(-1)), engine.match_within(b["emb"].reshape(-1, 512), min_cos, 2))
    engine.reset_counters()
    engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_WITHIN)
    assert engine.counters()["match_launches"] == 1      # a fused pass is one matcher launch


def _same_results(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert list(x.keys()) == list(y.keys())
            for k in x:
                assert np.array_equal(x[k], y[k]) if k == "embedding" else x[k] == y[k], (k, x[k], y[k])


@pytest.mark.parametrize("n_dup", [2, WITHIN_CAP + 6])
def test_service_all_matches_and_batch_compare_parity(fresh_engine, monkeypatch, n_dup):
    """FaceService on a real engine, near-duplicate identities so that a face has several hits: all_matches and
    batch_compare_faces (with and without target_names) give the same lists with use_within on and off; with more than 64
    duplicates of one identity the device lists are cut and the service falls back to the full rows"""
    monkeypatch.setenv("FRP_EXACT_COMPAT", "0")          # batch_compare_faces on the cosine rows (the exact branch is untouched)
    engine = fresh_engine
    rng = np.random.default_rng(99)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 4
    frames = _frames(rng, B, H, W)
    probe = engine.detect(frames, max_faces=K, det_thresh=1e-6)
    assert probe["counts"].min() >= 2
    thr = float(min(np.sort(probe["scores"][b, :probe["counts"][b]])[::-1][1] for b in range(B))) * 0.999
    fs = FaceService(engine=engine)
    assert not fs.ENCODINGS.exact and fs.use_within
    first = fs.process_frames(frames, max_faces=K, det_thresh=thr)           # empty gallery: the faces' embeddings
    e00, e10 = first[0][0]["embedding"], first[1][0]["embedding"]
    rows_by_name = {}
    for i in range(max(40, n_dup)):                                            # copies of face (0, 0) enrolled between distractors
        rows_by_name[f"x{i}"] = rng.standard_normal(512).astype(np.float32)
        if i < n_dup:
            rows_by_name[f"dup{i}"] = e00
    rows_by_name["near"] = e00 + 0.15 * rng.standard_normal(512).astype(np.float32) / np.sqrt(512)
    rows_by_name["other_face"] = e10
    names = list(rows_by_name)
    fs.ENCODINGS.set_bulk(names, np.stack([np.asarray(rows_by_name[nme], np.float32) for nme in names]))
    queries = [e00, e10, rows_by_name["x3"], rng.standard_normal(512).astype(np.float32)]
    subset = ["near", "dup1", "x3", "nobody", "dup0", "other_face"]
    got = {}
    for on in (True, False):
        fs.use_within = on
        got[on] = (fs.process_frames(frames, max_faces=K, det_thresh=thr, all_matches=True),
                   fs.batch_compare_faces(queries), fs.batch_compare_faces(queries, target_names=subset))
    _same_results(got[True][0], got[False][0])
    assert got[True][1] == got[False][1] and got[True][2] == got[False][2]
    m00 = [m["target"] for m in got[True][0][0][0]["matches"]]
    assert m00[:n_dup] == [f"dup{i}" for i in range(n_dup)] and "near" in m00[n_dup:]        # exact ties: enrolment order
    assert got[True][0][1][0]["matches"][0]["target"] == "other_face"
    assert [m["target"] for m in got[True][1][0]][:n_dup] == m00[:n_dup]
    assert [m["target"] for m in got[True][2][0]][:2] == ["dup1", "dup0"]                     # ties by position in target_names
    assert got[True][1][2][0]["target"] == "x3" and got[True][1][3] == []
