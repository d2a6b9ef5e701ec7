"""GPU tests of gallery groups (include/frp.h: frp_gallery_set_groups, frp_match_groups, frp_match_within_groups, FRP_FLAG_GROUPS /
frp_set_frame_groups; FaceService on top of them).  Expected values come from the float64 model alone - match_model.top1 / topk /
within on groups_cases.masked_scores(): the exact family's score matrix with NaN where a row is not permitted - and are compared
bit for bit (match_model.same_bits).  The conditions the mask patterns meet, and the wrong models they separate from the right one:
tests/test_groups_inputs.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import groups_cases as gc
import match_cases as mc
import match_model as mm
from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

ALL = gc.ALL


def _same_all(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if not mm.same_bits(g, w):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError((what, i, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _within_bounds(S):
    """the bounds of tests/test_gpu_match_exact.py, taken on the unmasked scores (the second one equals a score: `>=` is exercised)"""
    neg = 0 if S.shape[0] == 1 else mc.Q_NEGATIVE
    return [1.0, float(S[neg].max()), 0.0, -2.0]


@functools.lru_cache(maxsize=None)
def _ref(N, M):
    """-> (G, Q, S float32 [M, N] unmasked, row masks, query masks, masked S); computed once per shape, read-only"""
    G, Q = mc.exact_case(N, M)
    S = gc.exact_scores(N, M)
    rg, qg = gc.row_groups(N), gc.query_groups(M)
    Sm = gc.masked_scores(S, rg, qg)
    Sm.setflags(write=False)
    return G, Q, S, rg, qg, Sm


def _install(engine, N, M):
    G, Q, S, rg, qg, Sm = _ref(N, M)
    engine.gallery_set(G)
    engine.gallery_set_groups(rg)
    return Q, S, qg, Sm


# ------------------------------------------------------------------------------------------------ the grouped matcher
@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_grouped_top1(engine, monkeypatch, N, M):
    Q, S, qg, Sm = _install(engine, N, M)
    want = mm.top1(Sm)
    _same_all(engine.match(Q, groups=qg), want, "match groups")
    if M == 1:                                                  # the second run of the single query: it permits nothing
        _same_all(engine.match(Q, groups=gc.query_groups_none(1)), (np.array([-1], np.int32), np.array([-2.0], np.float32)), "mask 0")
    _same_all(engine.match(Q), mm.top1(S), "the ungrouped match next to it")
    monkeypatch.setenv("FRP_MATCH_V1", "1")
    _same_all(engine.match(Q, groups=qg), want, "match groups, FRP_MATCH_V1")


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_grouped_topk(engine, N, M):
    Q, S, qg, Sm = _install(engine, N, M)
    idx, cos = mm.topk(Sm, 64)
    for k in (2, 7, 64):
        _same_all(engine.match(Q, topk=k, groups=qg), (np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(cos[:, :k])), f"topk {k}")
    _same_all((engine.match_scores(Q),), (S,), "match_scores ignores groups")


@pytest.mark.parametrize("N,M", mc.EXACT_SHAPES)
def test_grouped_within(engine, N, M):
    Q, S, qg, Sm = _install(engine, N, M)
    for min_cos in _within_bounds(S):
        idx, cos, n = mm.within(Sm, min_cos, 64)
        for cap in (64, 3):                                     # cap 3: lists overflow, the grouped rebuild
            want = (np.ascontiguousarray(idx[:, :cap]), np.ascontiguousarray(cos[:, :cap]), n)
            _same_all(engine.match_within(Q, min_cos, cap, groups=qg), want, f"within {min_cos} cap {cap}")
        if min_cos == -2.0 and N > 64:
            assert n.max() > 3                                   # (the rebuild ran)


@pytest.mark.parametrize("N,M", [(129, 33), (4097, 320), (300, 513)])
def test_all_masks_all_equals_ungrouped_and_all_masks_zero_matches_nothing(engine, N, M):
    G, Q, S, _, _, _ = _ref(N, M)
    engine.gallery_set(G)
    assert np.all(engine.gallery_get_groups() == ALL)          # rows arrive as members of every group
    _same_all(engine.match(Q, groups=ALL), mm.top1(S), "top-1, ALL / ALL")
    _same_all(engine.match(Q, topk=7, groups=ALL), mm.topk(S, 7), "top-7, ALL / ALL")
    _same_all(engine.match_within(Q, 0.0, 3, groups=ALL), mm.within(S, 0.0, 3), "within, ALL / ALL")
    engine.gallery_set_groups(np.zeros(N, np.uint32))
    none = np.full((M, 3), -1, np.int32), np.full((M, 3), -2.0, np.float32)
    _same_all(engine.match(Q, groups=ALL), (none[0][:, 0], none[1][:, 0]), "top-1, rows 0")
    _same_all(engine.match(Q, topk=3, groups=ALL), none, "top-3, rows 0")
    _same_all(engine.match_within(Q, -2.0, 3, groups=ALL), none + (np.zeros(M, np.int32),), "within, rows 0")
    _same_all(engine.match(Q), mm.top1(S), "the ungrouped match ignores the masks")


# ------------------------------------------------------------------------------------------------ row masks through gallery updates
def test_row_masks_follow_gallery_updates(fresh_engine):
    engine = fresh_engine
    N, M = 129, 33
    G, Q, S, rg, qg, _ = _ref(N, M)
    rows, masks = np.array(G), np.array(rg)                      # the numpy mirror of every move
    engine.gallery_set(G)
    assert np.all(engine.gallery_get_groups() == ALL)
    engine.gallery_set_groups(rg)
    engine.match(Q, groups=qg)                                   # (the device copy of the masks exists from here on: updates patch it)
    engine.gallery_set_groups(np.array([1 << 9, 1 << 1], np.uint32), first=40)
    masks[40:42] = [1 << 9, 1 << 1]
    engine.gallery_update_row(3, G[100])                         # overwrite: the row keeps its mask
    rows[3] = G[100]
    engine.gallery_update_row(N, G[7])                           # append: ALL
    rows, masks = np.concatenate([rows, G[7][None]]), np.concatenate([masks, [ALL]]).astype(np.uint32)
    engine.gallery_remove_row(11)                                # the last row (the appended one) moves into 11 with its mask
    rows[11], masks[11] = rows[-1], masks[-1]
    rows, masks = rows[:-1], masks[:-1]
    engine.gallery_remove_row(len(rows) - 1)                     # the last row itself
    rows, masks = rows[:-1], masks[:-1]
    engine.gallery_remove_row(0)
    rows[0], masks[0] = rows[-1], masks[-1]
    rows, masks = rows[:-1], masks[:-1]
    assert engine.gallery_size() == len(rows) == N - 2
    assert np.array_equal(engine.gallery_get_groups(), masks)
    assert np.array_equal(engine.gallery_get_groups(first=10, n=3), masks[10:13])
    _same_all((engine.gallery_get(),), (mc.unit16(rows),), "rows")
    Sm = gc.masked_scores(mm.scores(mc.unit16(rows), mc.unit16(Q)).astype(np.float32), masks, qg)
    _same_all(engine.match(Q, groups=qg), mm.top1(Sm), "top-1 after the moves")
    _same_all(engine.match_within(Q, 0.0, 64, groups=qg), mm.within(Sm, 0.0, 64), "within after the moves")
    n_app = 40                                                   # appends past the device mask table's capacity (it is rebuilt)
    for _ in range(n_app):
        engine.gallery_update_row(engine.gallery_size(), G[5])
    rows = np.concatenate([rows, np.repeat(G[5][None], n_app, axis=0)])
    masks = np.concatenate([masks, np.full(n_app, ALL)]).astype(np.uint32)
    assert np.array_equal(engine.gallery_get_groups(), masks)
    Sm = gc.masked_scores(mm.scores(mc.unit16(rows), mc.unit16(Q)).astype(np.float32), masks, qg)
    _same_all(engine.match(Q, groups=qg), mm.top1(Sm), "top-1 after appends")
    # a pending reservation blocks set_groups as it blocks the other updates
    engine.gallery_reserve(8)
    with pytest.raises(FrpError):
        engine.gallery_set_groups(np.zeros(2, np.uint32))
    engine.gallery_cancel()
    assert np.array_equal(engine.gallery_get_groups(), masks)


# ------------------------------------------------------------------------------------------------ refusals of the stand-alone calls
def test_grouped_match_refusals(engine):
    G, Q, _, rg, qg, _ = _ref(129, 33)
    engine.gallery_set(G)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib, h = engine._lib, engine._h
    q = np.ascontiguousarray(Q, np.float32)
    g = np.ascontiguousarray(qg)
    idx, cos, n = np.empty((33, 8), np.int32), np.empty((33, 8), np.float32), np.empty(33, np.int32)
    inv = -1                                                     # FRP_ERR_INVALID
    assert lib.frp_match_groups(h, ptr(q), 33, None, 1, ptr(idx), ptr(cos)) == inv
    assert lib.frp_match_groups(h, None, 33, ptr(g), 1, ptr(idx), ptr(cos)) == inv
    assert lib.frp_match_groups(h, ptr(q), 33, ptr(g), 1, None, ptr(cos)) == inv
    assert lib.frp_match_groups(h, ptr(q), 33, ptr(g), 1, ptr(idx), None) == inv
    for k in (0, native.MAX_TOPK + 1):
        assert lib.frp_match_groups(h, ptr(q), 33, ptr(g), k, ptr(idx), ptr(cos)) == inv
    assert lib.frp_match_within_groups(h, ptr(q), 33, None, 0.5, 8, ptr(idx), ptr(cos), ptr(n)) == inv
    assert lib.frp_match_within_groups(h, ptr(q), 33, ptr(g), 0.5, 8, ptr(idx), ptr(cos), None) == inv
    for cap in (0, 65):
        assert lib.frp_match_within_groups(h, ptr(q), 33, ptr(g), 0.5, cap, ptr(idx), ptr(cos), ptr(n)) == inv
    assert lib.frp_match_within_groups(h, ptr(q), 33, ptr(g), float("nan"), 8, ptr(idx), ptr(cos), ptr(n)) == inv
    assert lib.frp_match_within_groups(h, ptr(q), 33, ptr(g), -2.5, 8, ptr(idx), ptr(cos), ptr(n)) == inv
    out = np.empty(4, np.uint32)
    for first, cnt in ((-1, 2), (128, 2), (0, 130), (0, -1)):
        assert lib.frp_gallery_set_groups(h, ptr(out), first, cnt) == inv
        assert lib.frp_gallery_get_groups(h, ptr(out), first, cnt) == inv
    assert lib.frp_gallery_set_groups(h, None, 0, 2) == inv and lib.frp_gallery_get_groups(h, None, 0, 2) == inv
    assert lib.frp_set_frame_groups(h, None, 2) == inv and lib.frp_set_frame_groups(h, ptr(out), 0) == inv
    with pytest.raises(ValueError):
        engine.match(Q, groups=qg[:5])
    assert np.all(engine.gallery_get_groups() == ALL)            # nothing above changed a mask
    engine.gallery_set(np.zeros((0, 512), np.float32))
    with pytest.raises(FrpError, match="gallery is empty"):
        engine.match(Q, groups=qg)


def test_grouped_launch_counts_its_mask_bytes(engine):
    N, M = 4097, 320
    Q, S, qg, Sm = _install(engine, N, M)
    engine.reset_counters()
    engine.match(Q, groups=qg)
    c = engine.counters()
    assert c["match_launches"] == 1 and c["match_bytes"] == N * (1024 + 4)
    engine.reset_counters()
    engine.match(Q)
    assert engine.counters()["match_bytes"] == N * 1024


# ------------------------------------------------------------------------------------------------ the grouped pass
def _frames(rng, B, H, W):
    base = rng.integers(0, 255, size=(B, H // 16, W // 16, 3)).astype(np.float32)
    base = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    return np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)


def _planted(engine, rng, frames, K):
    """the gallery of tests/test_gpu_match_within.py - face (0, 0) of the engine's own embeddings at rows 10 and 400 (an exact tie) and,
    perturbed, at 650; face (1, 0) at row 5 - plus one more exact copy of face (0, 0) at row 300"""
    engine.gallery_set(np.zeros((0, 512), np.float32))
    e = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_NO_MATCH)["emb"]
    G = rng.standard_normal((700, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    G[400] = G[300] = G[10] = e[0, 0]
    G[650] = e[0, 0] + 0.1 * rng.standard_normal(512).astype(np.float32) / np.sqrt(512)
    G[5] = e[1, 0]
    return G


def _pass_setup(engine):
    rng = np.random.default_rng(2024)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 6
    frames = _frames(rng, B, H, W)
    engine.gallery_set(_planted(engine, rng, frames, K))
    probe = engine.detect(frames, max_faces=K, det_thresh=1e-6)
    sc = np.sort(probe["scores"][0, :probe["counts"][0]])[::-1]
    assert len(sc) >= 3
    thr = float(0.5 * (sc[1] + sc[2]))                   # frame 0 keeps two faces: empty slots, a count below the capacity
    return frames, K, thr


@pytest.mark.selfcheck
def test_grouped_pass_equals_plain_pass_and_grouped_match(fresh_engine):
    """FRP_FLAG_GROUPS changes nothing about a pass but its match, which is match(emb, groups = the mask of the face's frame) bit for
    bit - with the face count on the device (threshold mode) and on the host (forced-K), alone and together with FRP_FLAG_WITHIN"""
    engine = fresh_engine
    frames, K, thr = _pass_setup(engine)
    B = len(frames)
    row_masks = np.full(700, 1 << 0, np.uint32)
    row_masks[10] = 1 << 1                               # row 10 is out for frame 0; its exact duplicates 300 and 400 are in
    engine.gallery_set_groups(row_masks)
    frame_masks = np.array([1 << 0, 0], np.uint32)       # frame 1 looks for nobody
    min_cos, cap = 0.9, 8
    engine.set_within(min_cos, cap)
    engine.set_frame_groups(frame_masks)
    for flags, dt in ((0, thr), (native.FLAG_FORCED_K, 0.5)):
        a = engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags)
        b = engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags | native.FLAG_GROUPS)
        c = engine.process_frames(frames, max_faces=K, det_thresh=dt, flags=flags | native.FLAG_GROUPS | native.FLAG_WITHIN)
        idx, cos, n = engine.fetch_within()
        for k in ("counts", "boxes", "kps", "scores", "emb"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k
        live = np.arange(K)[None, :] < b["counts"][:, None]
        assert live[0].any() and live[1].any() and (flags or not live.all())
        face_mask = np.repeat(frame_masks[:, None], K, axis=1)[live]
        want = engine.match(b["emb"][live], groups=face_mask)
        for got in (b, c):
            _same_all((got["match_idx"][live], got["match_cos"][live]), want, f"pass top-1, flags {flags}")
            assert np.all(got["match_idx"][~live] == -1)
            assert np.all(got["match_idx"][1] == -1) and np.all(got["match_cos"][1][live[1]] == np.float32(-2.0))      # frame 1: nothing
        assert a["match_idx"][0, 0] == 10 and b["match_idx"][0, 0] == 300 and b["match_cos"][0, 0] == a["match_cos"][0, 0]
        assert a["match_idx"][1, 0] == 5
        _same_all((idx[live], cos[live], n[live]), engine.match_within(c["emb"][live], min_cos, cap, groups=face_mask), f"pass lists, flags {flags}")
        assert not n[~live].any() and not n[1].any() and np.all(idx[1] == -1)
        assert n[0, 0] >= 3 and idx[0, 0, :2].tolist() == [300, 400] and 650 in idx[0, 0] and 10 not in idx[0, 0]
    # a list that overflows is rebuilt at fetch time - grouped as well: rows 300 and 400, not row 10
    engine.set_within(min_cos, 2)
    c = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_GROUPS | native.FLAG_WITHIN)
    idx, cos, n = engine.fetch_within()
    assert n[0, 0] >= 3 and idx[0, 0].tolist() == [300, 400]
    face_mask = np.repeat(frame_masks, K)
    _same_all((idx.reshape(-1, 2), cos.reshape(-1, 2), n.reshape(-1)), engine.match_within(c["emb"].reshape(-1, 512), min_cos, 2, groups=face_mask),
              "rebuilt lists")
    engine.reset_counters()
    engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_GROUPS | native.FLAG_WITHIN)
    ctr = engine.counters()
    assert ctr["match_launches"] == 1 and ctr["match_bytes"] == 700 * (1024 + 4)      # a grouped pass is one matcher launch
    # the split entry points end in the same pass: resident, finish_faces, the pyramid
    engine.upload_frames(frames)
    engine.process_resident(K, flags=native.FLAG_FORCED_K | native.FLAG_GROUPS)
    r = engine.fetch_results()
    _same_all((r["match_idx"], r["match_cos"]), (c["match_idx"], c["match_cos"]), "process_resident")
    f = engine.finish_faces(c["boxes"], c["kps"], c["scores"], c["counts"], K, flags=native.FLAG_GROUPS)
    _same_all((f["match_idx"], f["match_cos"]), (c["match_idx"], c["match_cos"]), "finish_faces")
    engine.process_pyramid_resident([(192, 256)], per_scale=K, max_faces=K, det_thresh=thr, flags=native.FLAG_GROUPS)
    p = engine.fetch_results()
    plive = np.arange(K)[None, :] < p["counts"][:, None]
    assert plive[0].any() and plive[1].any()
    _same_all((p["match_idx"][plive], p["match_cos"][plive]), engine.match(p["emb"][plive], groups=np.repeat(frame_masks[:, None], K, axis=1)[plive]),
              "process_pyramid")


def test_grouped_pass_refusals_leave_the_last_pass_fetchable(fresh_engine):
    engine = fresh_engine
    frames, K, thr = _pass_setup(engine)
    fl = native.FLAG_FORCED_K
    a = engine.process_frames(frames, max_faces=K, flags=fl)
    engine.upload_frames(frames)                                  # (the resident-frame calls below are sized by it; the pass's results stay)

    def still_there():
        r = engine.fetch_results()
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), r[k].view(np.uint8)), k

    def refused(call):
        engine.reset_counters()
        with pytest.raises(FrpError) as e:
            call()
        assert e.value.code == -1                                 # FRP_ERR_INVALID
        ctr = engine.counters()
        assert ctr["match_launches"] == 0 and ctr["det_conv_launches"] == 0 and ctr["emb_conv_launches"] == 0      # nothing launched
        still_there()

    kps_ok = (a["boxes"], a["kps"], a["scores"], a["counts"], K)
    # without a preceding set_frame_groups
    refused(lambda: engine.process_frames(frames, max_faces=K, flags=fl | native.FLAG_GROUPS))
    refused(lambda: engine.process_resident(K, flags=fl | native.FLAG_GROUPS))
    refused(lambda: engine.finish_faces(*kps_ok, flags=native.FLAG_GROUPS))
    refused(lambda: engine.process_pyramid_resident([(192, 256)], per_scale=K, max_faces=K, flags=native.FLAG_GROUPS))
    # with masks for another B
    engine.set_frame_groups(np.full(3, ALL, np.uint32))
    refused(lambda: engine.process_frames(frames, max_faces=K, flags=fl | native.FLAG_GROUPS))
    refused(lambda: engine.process_resident(K, flags=fl | native.FLAG_GROUPS))
    refused(lambda: engine.finish_faces(*kps_ok, flags=native.FLAG_GROUPS))
    refused(lambda: engine.process_pyramid_resident([(192, 256)], per_scale=K, max_faces=K, flags=native.FLAG_GROUPS))
    # together with FRP_FLAG_NO_MATCH
    engine.set_frame_groups(np.full(2, ALL, np.uint32))
    refused(lambda: engine.process_frames(frames, max_faces=K, flags=fl | native.FLAG_GROUPS | native.FLAG_NO_MATCH))
    refused(lambda: engine.process_resident(K, flags=fl | native.FLAG_GROUPS | native.FLAG_NO_MATCH))
    # ... and with the masks of this B the flagged pass runs: every frame ALL is the plain pass
    b = engine.process_frames(frames, max_faces=K, flags=fl | native.FLAG_GROUPS)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the service
def test_service_groups_equal_a_gallery_cut_down_to_the_permitted_names(fresh_engine, monkeypatch):
    """FaceService.process_frames(groups=[...]) on the real engine: per frame the dicts the plain call returns for a gallery that
    holds the permitted names only - same targets in the same order, distances bit-equal - with the hit lists from the pass
    (use_within) and from full score rows"""
    from frp_amd.face_service import FaceService
    monkeypatch.setenv("FRP_EXACT_COMPAT", "0")
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
    first = fs.process_frames(frames, max_faces=K, det_thresh=thr)           # empty gallery: the faces' embeddings
    e00, e10 = first[0][0]["embedding"], first[1][0]["embedding"]
    A, Bm, Cm = 1 << 0, 1 << 1, 1 << 2
    rows, masks = {}, {}
    for i in range(12):
        rows[f"x{i}"], masks[f"x{i}"] = rng.standard_normal(512).astype(np.float32), (A, Bm, Cm)[i % 3]
    rows["dupA"], masks["dupA"] = e00, A                                    # the same face enrolled on three lists
    rows["dupB"], masks["dupB"] = e00, Bm
    rows["dupAC"], masks["dupAC"] = e00, A | Cm
    rows["near"], masks["near"] = e00 + 0.15 * rng.standard_normal(512).astype(np.float32) / np.sqrt(512), Bm
    rows["other"], masks["other"] = e10, Cm
    rows["suspended"], masks["suspended"] = e10, 0
    names = list(rows)
    mat = np.stack([np.asarray(rows[n], np.float32) for n in names])
    frame_masks = [Bm, A | Cm]                                              # frame 0 looks for list B, frame 1 for lists A and C
    got = {}
    for on in (True, False):
        fs.use_within = on
        fs.ENCODINGS.set_bulk(names, mat, groups=[masks[n] for n in names])
        assert [fs.ENCODINGS.groups_of(n) for n in names] == [masks[n] for n in names]
        assert np.array_equal(engine.gallery_get_groups(), np.array([masks[n] for n in names], np.uint32))
        got[on] = fs.process_frames(frames, max_faces=K, det_thresh=thr, all_matches=True, groups=frame_masks)
        for b, fm in enumerate(frame_masks):
            keep = [n for n in names if masks[n] & fm]
            fs.ENCODINGS.set_bulk(keep, np.stack([np.asarray(rows[n], np.float32) for n in keep]))
            want = fs.process_frames(frames, max_faces=K, det_thresh=thr, all_matches=True)[b]
            assert len(got[on][b]) == len(want) >= 2
            for x, y in zip(got[on][b], want):
                assert list(x.keys()) == list(y.keys())
                for k in x:
                    assert np.array_equal(x[k], y[k]) if k == "embedding" else x[k] == y[k], (on, b, k, x[k], y[k])
    def listed(face):
        return [m["target"] for m in face["matches"]]

    # (the synthetic embedder's faces lie close to each other: a face also lists the other face's identities, where permitted)
    assert got[True][0][0]["target"] == "dupB" and listed(got[True][0][0])[:2] == ["dupB", "near"]
    assert got[True][1][0]["target"] == "other" and listed(got[True][1][0])[0] == "other"
    for b, fm in enumerate(frame_masks):
        for face in got[True][b]:
            assert all(masks[t] & fm for t in listed(face)) and (face["target"] is None or masks[face["target"]] & fm)
    assert got[True][0][0]["matches"] == got[False][0][0]["matches"]
    # an identity moved to another list, a mask per call for all frames
    fs.ENCODINGS.set_bulk(names, mat, groups=[masks[n] for n in names])
    fs.ENCODINGS.set_groups("dupB", Cm)
    assert fs.store_face("late", e00, groups=Bm)["success"]
    out = fs.process_frames(frames, max_faces=K, det_thresh=thr, all_matches=True, groups=Bm)
    assert listed(out[0][0])[:2] == ["late", "near"] and out[0][0]["target"] == "late" and "dupB" not in listed(out[0][0])
    assert fs.delete_face("x0")["success"]                                 # swap-remove: host table and device masks move alike
    assert np.array_equal(engine.gallery_get_groups(), fs.ENCODINGS.groups_table())
