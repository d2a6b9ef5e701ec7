"""CPU tests of the host half of the radius match: the helper that turns a device hit list into the sorted match list, the
cosine bound derived from a distance tolerance, and FaceService on engines with and without `match_within` (tests/fake_engine.py
has none: all_matches and batch_compare_faces keep the full-row path there)."""
import numpy as np
import pytest

from fake_engine import FakeEngine
from frp_amd import native
from frp_amd.face_service import (WITHIN_CAP, FaceService, confidence_level, cos_to_distance, within_min_cos,
                                  within_to_matches)


def test_within_to_matches_orders_by_distance_then_name_position():
    # rows 5, 9 and 2 tie exactly; their names sit at positions 3, 0 and 7: the tie must come out as 9, 5, 2
    pos_of_row = np.full(12, -1, np.int64)
    pos_of_row[[5, 9, 2, 4, 11]] = [3, 0, 7, 1, 2]
    rows = np.array([5, 9, 2, 4, 11, -1, -1, -1], np.int32)            # device order: (cosine desc, row asc), padded
    cos = np.array([0.95, 0.95, 0.95, 0.90, 0.70, -2.0, -2.0, -2.0], np.float32)
    cos[:3] = np.float32(0.95)
    rows[:3] = [2, 5, 9]
    tol = 0.6
    got = within_to_matches(rows, cos, 5, tol, pos_of_row)
    d = cos_to_distance(cos[:5])
    assert [p for p, _ in got] == [0, 3, 7, 1]                           # ties by position; row 11 (d = 0.77) is beyond tol
    assert [x for _, x in got] == [d[0], d[0], d[0], d[3]]
    assert all(isinstance(x, float) for _, x in got)
    # the same answer as the full-row path: a stable argsort over distances laid out by position
    full = np.full(8, 9.0)
    full[pos_of_row[rows[:5]]] = d
    order = [j for j in np.argsort(full, kind="stable") if full[j] <= tol]
    assert [p for p, _ in got] == order
    # a true count beyond the list length reads only what the list holds; zero hits and rows outside the target subset drop out
    assert within_to_matches(rows[:2], cos[:2], 66, tol, pos_of_row) == [(3, d[0]), (7, d[0])]
    assert within_to_matches(rows, cos, 0, tol, pos_of_row) == []
    pos_of_row[5] = -1
    assert [p for p, _ in within_to_matches(rows, cos, 5, tol, pos_of_row)] == [0, 7, 1]


@pytest.mark.parametrize("tol", [0.0, 1e-3, 0.3, 0.4, 0.5, 0.6, 0.9, 1.0, 1.3, 1.99, 2.0])
def test_within_min_cos_never_excludes_a_row_the_host_test_accepts(tol):
    """every float32 cosine with cos_to_distance(cos) <= tol is >= the bound (walk the float32 values around 1 - tol^2 / 2)"""
    m = within_min_cos(tol)
    assert m == np.float32(m) and m >= -2.0
    c = np.float32(1.0 - 0.5 * tol * tol)
    near = [c]
    for _ in range(64):
        near.append(np.nextafter(near[-1], np.float32(-np.inf)))
    lo = c
    for _ in range(64):
        lo = np.nextafter(lo, np.float32(np.inf))
        near.append(lo)
    near = np.array(near, np.float32)
    accepted = near[cos_to_distance(near) <= tol]
    assert accepted.size and np.all(accepted >= np.float32(m))
    assert 1.0 - 0.5 * tol * tol - m < 1e-5                              # and it is only just below the exact bound


def test_within_min_cos_wide_tolerances_list_everything():
    assert within_min_cos(2.5) == -2.0 and within_min_cos(100.0) == -2.0 and within_min_cos(float("nan")) == -2.0


class WithinEngine(FakeEngine):
    """FakeEngine + the radius-match calls in numpy, on float32 scores as the device returns them"""

    def __init__(self):
        super().__init__()
        self.flags_seen = []
        self.within_calls = 0
        self.score_calls = 0

    def match_scores(self, q):
        self.score_calls += 1
        return super().match_scores(q).astype(np.float32)

    def match_within(self, q, min_cos, cap=64):
        self.within_calls += 1
        S = FakeEngine.match_scores(self, q).astype(np.float32)
        M = len(S)
        idx = np.full((M, cap), -1, np.int32)
        cos = np.full((M, cap), -2.0, np.float32)
        n = np.zeros(M, np.int32)
        for i in range(M):
            order = [j for j in np.argsort(-S[i].astype(np.float64), kind="stable") if S[i, j] >= np.float32(min_cos)]
            n[i] = len(order)
            k = min(len(order), cap)
            idx[i, :k] = order[:k]
            cos[i, :k] = S[i, order[:k]]
        return idx, cos, n

    def set_within(self, min_cos, cap=64):
        self._within = (min_cos, cap)

    def process_frames(self, frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.flags_seen.append(flags)
        return self.canned

    def fetch_within(self):
        min_cos, cap = self._within
        B, K = self.canned["counts"].shape[0], self.canned["match_idx"].shape[1]
        idx = np.full((B, K, cap), -1, np.int32)
        cos = np.full((B, K, cap), -2.0, np.float32)
        n = np.zeros((B, K), np.int32)
        for b in range(B):
            c = int(self.canned["counts"][b])
            if c:
                idx[b, :c], cos[b, :c], n[b, :c] = self.match_within(self.canned["emb"][b, :c], min_cos, cap)
        return idx, cos, n


def _gallery(n_dup):
    """unit rows: `n_dup` copies of one direction (names d0, d1, ... enrolled in an order unlike their rows' cosine order), two
    near copies of another, and unrelated rows"""
    rng = np.random.default_rng(5)
    base = rng.standard_normal((4, 512))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rows, names = [], []
    for i in range(n_dup):
        rows.append(base[0])
        names.append(f"d{i}")
    for i in range(2):
        v = base[1] + 0.02 * (i + 1) * base[3]
        rows.append(v / np.linalg.norm(v))
        names.append(f"near{i}")
    rows.append(base[2])
    names.append("other")
    return base, np.array(rows), names


def _canned(base):
    B, K = 2, 3
    emb = np.zeros((B, K, 512), np.float32)
    emb[0, 0], emb[0, 1], emb[1, 0] = base[0], base[1], base[3]
    return dict(boxes=np.zeros((B, K, 4), np.float32), kps=np.zeros((B, K, 5, 2), np.float32), scores=np.ones((B, K), np.float32),
                counts=np.array([2, 1], np.int32), emb=emb, match_idx=np.array([[0, 3, -1], [-1, -1, -1]], np.int32),
                match_cos=np.array([[1.0, 0.99, -1], [-1, -1, -1]], np.float32))


def _service(monkeypatch, eng, n_dup):
    monkeypatch.setenv("FRP_EXACT_COMPAT", "0")              # the cosine branch of the compat calls (the exact one never changes)
    base, rows, names = _gallery(n_dup)
    fs = FaceService(engine=eng)
    assert not fs.ENCODINGS.exact
    for n, r in zip(names, rows):
        assert fs.store_face(n, r)["success"]
    eng.canned = _canned(base)
    return fs, base, names


def test_fake_engine_without_match_within_keeps_the_full_row_path(monkeypatch):
    eng = FakeEngine()
    assert not hasattr(eng, "match_within") and not hasattr(eng, "fetch_within")
    fs, base, names = _service(monkeypatch, eng, 3)
    assert fs.use_within
    out = fs.process_frames(np.zeros((2, 8, 8, 3), np.uint8), max_faces=3, all_matches=True)
    assert [len(f) for f in out] == [2, 1]
    assert [m["target"] for m in out[0][0]["matches"]] == ["d0", "d1", "d2"]          # exact ties: enrolment order
    assert [m["target"] for m in out[0][1]["matches"]] == ["near0", "near1"]
    assert out[1][0]["matches"] == []
    for m in out[0][0]["matches"] + out[0][1]["matches"]:
        assert list(m.keys()) == ["target", "distance", "confidence"] and m["confidence"] == confidence_level(m["distance"])
    res = fs.batch_compare_faces([base[0], base[1], base[3]])
    assert [[m["target"] for m in r] for r in res] == [["d0", "d1", "d2"], ["near0", "near1"], []]
    assert list(res[0][0].keys()) == ["target", "match", "distance", "confidence"] and res[0][0]["match"] is True
    sub = fs.batch_compare_faces([base[0]], target_names=["near0", "d2", "nobody", "d0"])
    assert [m["target"] for m in sub[0]] == ["d2", "d0"]                            # ties by position in target_names


@pytest.mark.parametrize("n_dup", [3, WITHIN_CAP, WITHIN_CAP + 2])
def test_service_on_the_radius_match_equals_the_full_row_path(monkeypatch, n_dup):
    """an engine with match_within / fetch_within: the same result lists with use_within on and off, the FLAG_WITHIN pass and no
    score matrix when on, and the full-row path again when a face has more hits than a list holds"""
    eng = WithinEngine()
    fs, base, names = _service(monkeypatch, eng, n_dup)
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    queries = [base[0], base[1], base[3]]
    subset = ["near1", "d2", "nobody", "d0", "near0"]
    got = {}
    for on in (True, False):
        fs.use_within = on
        eng.flags_seen.clear()
        eng.score_calls = eng.within_calls = 0
        pf = fs.process_frames(frames, max_faces=3, all_matches=True)
        assert bool(eng.flags_seen[-1] & native.FLAG_WITHIN) == on
        plain = fs.process_frames(frames, max_faces=3)
        assert not eng.flags_seen[-1] & native.FLAG_WITHIN and "matches" not in plain[0][0]
        got[on] = (pf, fs.batch_compare_faces(queries), fs.batch_compare_faces(queries, target_names=subset))
        overflow = n_dup > WITHIN_CAP
        if on and not overflow:
            assert eng.score_calls == 0 and eng.within_calls > 0
        else:
            assert eng.score_calls == 3                                           # one per call: the full rows
    for a, b in zip(got[True][0], got[False][0]):
        assert len(a) == len(b)
        for fa, fb in zip(a, b):
            assert list(fa.keys()) == list(fb.keys())
            for k in fa:
                assert np.array_equal(fa[k], fb[k]) if k == "embedding" else fa[k] == fb[k], k
    assert got[True][1] == got[False][1] and got[True][2] == got[False][2]
    assert [m["target"] for m in got[True][0][0][0]["matches"]] == [f"d{i}" for i in range(n_dup)]
    assert [m["target"] for m in got[True][2][0]] == ["d2", "d0"]
    # a name listed twice has two positions: the full-row path, which lists it twice
    fs.use_within = True
    eng.score_calls = 0
    twice = fs.batch_compare_faces([base[1]], target_names=["near0", "near0"])
    assert [m["target"] for m in twice[0]] == ["near0", "near0"] and eng.score_calls == 1
