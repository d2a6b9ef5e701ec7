"""CPU half of the device pyramid pass: the planted case list (tests/pyramid_cases.py) reaches every branch the merge kernel
can get wrong - shown with pyramid.merge_scales itself, the reference the kernel is held to - and FaceService carries
`det_scales` to the engine (validation, the three branches, None = the old calls) on a recording fake engine."""
import contextlib
from fractions import Fraction

import numpy as np
import pytest

from frp_amd import native, pyramid
from frp_amd.face_service import PYRAMID_PER_SCALE, FaceService
from frp_amd.yuv import YuvBatch, YuvFrame

from fake_engine import FakeEngine
from pyramid_cases import CASES, JUNK, per_scale, reference

f32 = np.float32


def _case(name):
    return next(c for c in CASES if c["name"] == name)


def _subset(case, b, picks):
    """merge_scales input that holds only the candidates `picks` = [(scale, row)] of frame b, in their order within each scale"""
    out = []
    for s, hw in enumerate(case["det_hws"]):
        rows = np.array(sorted(j for (ss, j) in picks if ss == s), dtype=np.int64)
        n = len(rows)
        out.append((hw, dict(boxes=case["boxes"][s, b:b + 1, rows].reshape(1, n, 4), kps=case["kps"][s, b:b + 1, rows].reshape(1, n, 5, 2),
                             scores=case["scores"][s, b:b + 1, rows].reshape(1, n), counts=np.array([n], np.int32))))
    return out


def _merge(case, b, picks, K):
    return pyramid.merge_scales(_subset(case, b, picks), case["frame_hw"], K, case["nms_iou"])


def _candidates(case, b):
    """[(scale, row)] of frame b in concatenated order"""
    return [(s, j) for s in range(len(case["det_hws"])) for j in range(int(case["counts"][s, b]))]


def _survivors(case, b):
    """the candidates that survive the merge without the K cut, in output order: every output row is identified through
    merge_scales of the one candidate alone (its mapped box, landmarks and score)"""
    cands = _candidates(case, b)
    S, P = case["scores"].shape[0], case["scores"].shape[2]
    ob, ok, osc, oc = reference(case, S * P)
    alone = {c: _merge(case, b, [c], 1) for c in cands}
    used, out = set(), []
    for r in range(int(oc[b])):
        hit = next(c for c in cands if c not in used and np.array_equal(alone[c][0][0, 0], ob[b, r]) and
                   np.array_equal(alone[c][1][0, 0], ok[b, r]) and alone[c][2][0, 0] == osc[b, r])
        used.add(hit)
        out.append(hit)
    return out


def _before(case, b, c, d):
    """candidate c sorts before d: score descending, ties to the lower concatenated index"""
    sc, sd = case["scores"][c[0], b, c[1]], case["scores"][d[0], b, d[1]]
    return sc > sd or (sc == sd and c < d)


def _planted_frames():
    return [(c, b) for c in CASES if c["name"].startswith(("planted_", "inexact_")) for b in range(c["counts"].shape[1])]


def test_case_list_is_small_and_well_formed():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        S, B, P = c["scores"].shape
        assert c["frame_hw"] in ((360, 500), (359, 501)) and B <= 3 and 1 <= S <= 4 and S * P <= 512 and 1 <= c["K"] <= 128
        assert c["boxes"].shape == (S, B, P, 4) and c["kps"].shape == (S, B, P, 5, 2) and c["counts"].shape == (S, B)
        assert all(a.dtype == f32 for a in (c["boxes"], c["kps"], c["scores"])) and c["counts"].dtype == np.int32
        assert c["counts"].min() >= 0 and c["counts"].max() <= P
        live = np.arange(P)[None, None, :] < c["counts"][:, :, None]
        assert np.isfinite(c["scores"][live]).all() and (c["scores"][live] >= 0).all()
        assert np.all(c["scores"][~live] == JUNK) and np.all(c["boxes"][~live] == JUNK)       # dead rows hold junk nobody may read
        ob, ok, osc, oc = reference(c)
        for b in range(B):                                                                     # ... and the reference does not
            n = int(oc[b])
            assert np.abs(ob[b, :n]).max(initial=0) < 1000 and np.all(ob[b, n:] == 0) and np.all(ok[b, n:] == 0) and np.all(osc[b, n:] == 0)


def test_a_box_is_suppressed_by_a_box_of_another_scale():
    found = 0
    for case, b in _planted_frames():
        kept = _survivors(case, b)
        for c in (c for c in _candidates(case, b) if c not in kept):
            sup = [m for m in kept if _before(case, b, m, c) and int(_merge(case, b, [m, c], 2)[3][0]) == 1]
            assert sup, "a candidate that did not survive has a survivor that suppresses it"
            if all(m[0] != c[0] for m in sup):
                found += 1
                break
    assert found >= 8


def test_equal_scores_within_and_across_scales_and_their_order_shows():
    within = across = 0
    for case, b in _planted_frames():
        assert np.all(case["scores"][0, b, :case["counts"][0, b]] * 16 % 1 == 0)              # sixteenths
        kept = _survivors(case, b)
        for c, d in zip(kept, kept[1:]):
            assert _before(case, b, c, d)
            if case["scores"][c[0], b, c[1]] == case["scores"][d[0], b, d[1]]:
                assert c < d                                                                   # scale order, then detector order
                within += c[0] == d[0]
                across += c[0] != d[0]
    assert within >= 5 and across >= 5


def test_the_k_cut_and_the_empty_frames():
    cut = 0
    one_scale_empty = all_empty = False
    for case, b in _planted_frames():
        S, P = case["scores"].shape[0], case["scores"].shape[2]
        n_all, n_k = int(reference(case, S * P)[3][b]), int(reference(case)[3][b])
        assert n_k == min(n_all, case["K"])
        cut += n_all > case["K"]
        cnt = case["counts"][:, b]
        one_scale_empty |= bool((cnt == 0).any() and (cnt > 0).any() and n_k > 0)
        all_empty |= bool((cnt == 0).all() and n_k == 0)
    assert cut >= 10 and one_scale_empty and all_empty


def test_iou_equal_to_the_threshold_is_kept_and_one_step_above_is_not():
    case = _case("exact_iou")
    assert case["nms_iou"] == 0.5 and f32(360) / f32(180) == 2 and f32(500) / f32(250) == 2
    ob, ok, osc, oc = reference(case)
    assert oc.tolist() == [3, 1, 0]

    def iou(b):                                       # the arithmetic of merge_scales on the mapped pair of frame b
        (x1, y1, x2, y2), (u1, v1, u2, v2) = _merge(case, b, [(0, 0)], 1)[0][0, 0], _merge(case, b, [(1, 0)], 1)[0][0, 0]
        a, c = (x2 - x1 + f32(1)) * (y2 - y1 + f32(1)), (u2 - u1 + f32(1)) * (v2 - v1 + f32(1))
        inter = max(f32(0), min(x2, u2) - max(x1, u1) + f32(1)) * max(f32(0), min(y2, v2) - max(y1, v1) + f32(1))
        return f32(inter / ((a + c) - inter))
    assert iou(0) == f32(0.5) and int(_merge(case, 0, [(0, 0), (1, 0)], 2)[3][0]) == 2
    assert iou(1) == np.nextafter(f32(0.5), f32(1)) and int(_merge(case, 1, [(0, 0), (1, 0)], 2)[3][0]) == 1
    assert np.array_equal(ob[0, 1], [0, 0, 8, 8])     # the half scale's integer box, mapped
    # a score of exactly 0.0 on a live row: kept, last
    assert case["scores"][0, 0, 1] == 0 and case["counts"][0, 0] == 2
    assert osc[0, 2] == 0 and np.array_equal(ob[0, 2], case["boxes"][0, 0, 1]) and np.all(ob[0, 3] == 0)


def test_single_scale_full_capacity_and_inexact_ratios():
    case = _case("single_scale")
    assert case["det_hws"] == [case["frame_hw"]]
    ob, ok, osc, oc = reference(case)
    for b in range(2):
        n = min(int(case["counts"][0, b]), case["K"])
        assert oc[b] == n and (case["counts"][0, 0] > case["K"] > case["counts"][0, 1])
        assert np.array_equal(ob[b, :n], case["boxes"][0, b, :n]) and np.array_equal(ok[b, :n], case["kps"][0, b, :n])
        assert np.array_equal(osc[b, :n], case["scores"][0, b, :n])
    case = _case("capacity_4x128")
    assert case["scores"].shape == (4, 2, 128) and np.all(case["counts"][:, 0] == 128) and case["K"] == 128
    assert 0 < int(reference(case)[3][1]) < int(reference(case)[3][0]) <= 128
    for case in (c for c in CASES if c["name"].startswith("inexact_")):
        assert case["frame_hw"] == (359, 501) and case["det_hws"] == [(359, 501), (180, 250), (90, 125)]      # scaled_size rounds
        for (hs, ws) in case["det_hws"][1:]:
            assert Fraction(float(f32(359) / f32(hs))) != Fraction(359, hs) and Fraction(float(f32(501) / f32(ws))) != Fraction(501, ws)
        assert int(reference(case)[3].min()) > 0


# ---------------------------------------------------------------- FaceService: det_scales on a recording engine
def _canned(B, K):
    return dict(boxes=np.zeros((B, K, 4), f32), kps=np.zeros((B, K, 5, 2), f32), scores=np.zeros((B, K), f32),
                counts=np.zeros((B,), np.int32), emb=np.zeros((B, K, 512), f32), match_idx=np.full((B, K), -1, np.int32),
                match_cos=np.full((B, K), -1.0, f32))


class OldEngine(FakeEngine):
    """records its hot-path calls; has no process_pyramid_resident"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def process_frames(self, frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_frames", dict(max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        return _canned(len(frames), max_faces)


class PlainEngine(OldEngine):
    def process_pyramid_resident(self, det_hws, per_scale=64, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_pyramid_resident", dict(det_hws=[tuple(hw) for hw in det_hws], per_scale=per_scale, max_faces=max_faces,
                                                            det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        self._k = max_faces

    def process_frames_pyramid(self, frames, scales=(1.0, 0.5, 0.25), max_faces=10, det_thresh=0.5, nms_iou=0.4, per_scale=64, flags=0,
                               on_device=False):
        self.calls.append(("process_frames_pyramid", dict(scales=tuple(scales), max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou,
                                                          per_scale=per_scale, flags=flags, on_device=on_device)))
        return _canned(len(frames), max_faces)


class StagedEngine(PlainEngine):
    """... with the staged-ingest calls of native.Engine"""

    def sequence(self):
        return contextlib.nullcontext()

    def upload_yuv_async(self, batch):
        self.calls.append(("upload_yuv_async", len(batch)))
        self._b = len(batch)

    def upload_frames_async(self, frames):
        self.calls.append(("upload_frames_async", len(frames)))
        self._b = len(frames)

    def swap_frames(self):
        self.calls.append(("swap_frames", None))

    def process_resident(self, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_resident", dict(max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        self._k = max_faces

    def fetch_results(self):
        self.calls.append(("fetch_results", None))
        return _canned(self._b, self._k)


def _frames(B=2, H=360, W=500):
    return np.zeros((B, H, W, 3), np.uint8)


def _yuv(B=2, H=360, W=500):
    return YuvBatch([YuvFrame(np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8)) for _ in range(B)], "NV12", "BT601")


@pytest.mark.parametrize("bad", [(), (1.0, 0.5, 0.25, 0.75, 0.6), (0.0,), (1.0, -0.5), (2.5,), (float("nan"),), 0.5])
def test_det_scales_are_validated_before_anything_reaches_the_engine(bad):
    eng = StagedEngine()
    svc = FaceService(engine=eng)
    with pytest.raises(ValueError, match="det_scales"):
        svc.process_frames(_frames(), det_scales=bad)
    with pytest.raises(ValueError, match="det_scales"):
        svc.process_frames(_yuv(), det_scales=bad)
    with pytest.raises(ValueError, match="det_scales"):
        svc.process_stream([_frames()], det_scales=bad)
    assert eng.calls == []
    assert 4 * PYRAMID_PER_SCALE <= 512          # (four scales always fit the merge kernel's 512 candidates)


def test_det_scales_on_an_engine_without_the_pass_names_the_attribute():
    eng = OldEngine()
    svc = FaceService(engine=eng)
    with pytest.raises(ValueError, match="process_pyramid_resident"):
        svc.process_frames(_frames(), det_scales=(1.0, 0.5))
    assert eng.calls == []
    assert svc.process_frames(_frames(), det_scales=None) == [[], []]
    assert [c[0] for c in eng.calls] == ["process_frames"]


def test_det_scales_reach_the_engine_in_the_plain_and_the_staged_branch():
    from frp_amd.face_service import DET_THRESH, NMS_IOU
    eng = PlainEngine()
    svc = FaceService(engine=eng)
    assert svc.process_frames(_frames(), max_faces=6, det_scales=[1, 0.5]) == [[], []]
    assert eng.calls == [("process_frames_pyramid", dict(scales=(1.0, 0.5), max_faces=6, det_thresh=DET_THRESH, nms_iou=NMS_IOU,
                                                         per_scale=PYRAMID_PER_SCALE, flags=native.FLAG_NO_MATCH, on_device=True))]
    eng.calls.clear()
    assert svc.process_frame(_frames()[0], metadata={"max_faces": 3, "det_scales": (0.5,)}) == []
    assert eng.calls[0][0] == "process_frames_pyramid" and eng.calls[0][1]["scales"] == (0.5,) and eng.calls[0][1]["max_faces"] == 3
    # staged (a YuvBatch on an engine with the device converter): upload, swap, ONE pyramid pass with the sizes of scaled_size, fetch
    eng = StagedEngine()
    svc = FaceService(engine=eng)
    assert svc.process_frames(_yuv(2, 360, 500), max_faces=5, det_scales=(1.0, 0.5, 0.25)) == [[], []]
    want = dict(det_hws=[pyramid.scaled_size(360, 500, s) for s in (1.0, 0.5, 0.25)], per_scale=PYRAMID_PER_SCALE, max_faces=5,
                det_thresh=DET_THRESH, nms_iou=NMS_IOU, flags=native.FLAG_NO_MATCH)
    assert eng.calls == [("upload_yuv_async", 2), ("swap_frames", None), ("process_pyramid_resident", want), ("fetch_results", None)]
    assert want["det_hws"] == [(360, 500), (180, 250), (90, 125)]
    # overlapped (process_stream): the pyramid pass in place of process_resident, every batch
    eng.calls.clear()
    out = list(svc.process_stream([_frames(2, 120, 160), _frames(2, 120, 160)], max_faces=4, det_scales=(0.5,)))
    assert out == [[[], []], [[], []]]
    passes = [c for c in eng.calls if c[0] in ("process_resident", "process_pyramid_resident", "process_frames")]
    assert [c[0] for c in passes] == ["process_pyramid_resident"] * 2 and passes[0][1]["det_hws"] == [(60, 80)] and passes[0][1]["max_faces"] == 4


def test_without_det_scales_the_old_calls_are_made_unchanged():
    from frp_amd.face_service import DET_THRESH, NMS_IOU
    old = dict(max_faces=10, det_thresh=DET_THRESH, nms_iou=NMS_IOU, flags=native.FLAG_NO_MATCH)
    eng = PlainEngine()
    assert FaceService(engine=eng).process_frames(_frames()) == [[], []]
    assert eng.calls == [("process_frames", old)]
    eng = StagedEngine()
    svc = FaceService(engine=eng)
    assert svc.process_frames(_yuv(), det_scales=None) == [[], []]
    assert eng.calls == [("upload_yuv_async", 2), ("swap_frames", None), ("process_resident", old), ("fetch_results", None)]
    eng.calls.clear()
    assert list(svc.process_stream([_frames(2, 120, 160)])) == [[[], []]]
    assert [c for c in eng.calls if c[0].startswith("process")] == [("process_resident", old)]
    eng.calls.clear()
    assert svc.process_frame(_frames()[0], metadata={"max_faces": 10}) == []
    assert [c[0] for c in eng.calls] == ["process_frames"]
