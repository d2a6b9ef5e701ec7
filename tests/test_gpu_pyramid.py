"""The detection pyramid as one device pass (frp_process_pyramid, pyramid_merge_kernel): held to pyramid.merge_scales and to the
host route (detect_resident per scale + merge_scales + finish_faces) bit for bit - never to itself."""
import numpy as np
import pytest

from frp_amd import native, pyramid
from frp_amd.face_service import NMS_IOU, PYRAMID_PER_SCALE, FaceService
from frp_amd.native import FrpError

from conftest import get_raw_and_blob
from pyramid_cases import CASES, reference

pytestmark = pytest.mark.gpu

KEYS = ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos")
SCALES, THR, K = (1.0, 0.5, 0.25), 0.30, 8


def _frames(rng, B, H, W):
    base = rng.normal(110, 12, size=(B, H, W, 3))
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(3):
            cx, cy, r = rng.uniform(30, W - 30), rng.uniform(30, H - 30), rng.uniform(15, 40)
            m = ((xx - cx) / r) ** 2 + ((yy - cy) / (1.3 * r)) ** 2 < 1
            base[b][m] += rng.uniform(30, 80)
    return np.clip(base, 0, 255).astype(np.uint8)


_INPUT = {}


def _input(hw=(360, 500)):
    """seed 99: the frames of test_resize_and_pyramid_merge (it asserts >= 2 faces per frame at 0.30) and a 64-row gallery"""
    if hw not in _INPUT:
        rng = np.random.default_rng(99)
        frames = _frames(rng, 2, *hw)
        _INPUT[hw] = (frames, rng.standard_normal((64, 512)).astype(np.float32))
    return _INPUT[hw]


def _ready(eng, hw=(360, 500)):
    frames, G = _input(hw)
    eng.load_weights(get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))[1])
    eng.gallery_set(G)
    return frames


def _same(got, want, keys=KEYS, what=""):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merge_kernel_equals_merge_scales(engine, case):
    got = engine.pyramid_merge(case["det_hws"], case["frame_hw"], case["boxes"], case["kps"], case["scores"], case["counts"],
                               case["K"], case["nms_iou"])
    want = reference(case)
    for name, g, w in zip(("boxes", "kps", "scores", "counts"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (case["name"], name)
    for b, n in enumerate(got[3]):                       # slots beyond the count are zero
        assert not got[0][b, n:].any() and not got[1][b, n:].any() and not got[2][b, n:].any()


@pytest.mark.parametrize("hw", [(360, 500), (359, 501)])
def test_whole_pass_equals_the_host_route(engine, monkeypatch, hw):
    """B x K = 16 slots is below FRP_WINO_MIN_FACES: both routes take the same embedder family; the host route launches for the
    count it knows, the device route for the capacity with the count in device memory - the same bits
    (test_threshold_mode_face_count_stays_on_the_device)"""
    frames = _ready(engine, hw)
    want = engine.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, nms_iou=0.4)
    got = engine.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, nms_iou=0.4, on_device=True)
    assert want["counts"].min() >= 2 and want["counts"].max() <= K
    _same(got, want, what=hw)
    live = np.arange(K)[None, :] < want["counts"][:, None]
    assert np.all(got["match_idx"][live] >= 0) and np.all(got["match_idx"][~live] == -1) and not got["emb"][~live].any()
    monkeypatch.setenv("FRP_HOST_COUNT", "1")            # the device route with the count copied to the host: the same again
    _same(engine.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, nms_iou=0.4, on_device=True), want, what="host count")
    monkeypatch.delenv("FRP_HOST_COUNT")
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_one_scale_equals_detect_merge_finish(engine):
    frames = _ready(engine)
    H, W = frames.shape[1:3]
    hw = pyramid.scaled_size(H, W, 0.5)
    engine.upload_frames(frames)
    d = engine.detect_resident(hw, max_faces=64, det_thresh=THR, nms_iou=0.4)
    boxes, kps, scores, counts = pyramid.merge_scales([(hw, d)], (H, W), K, 0.4)
    want = engine.finish_faces(boxes, kps, scores, counts, K)
    got = engine.process_frames_pyramid(frames, (0.5,), max_faces=K, det_thresh=THR, nms_iou=0.4, on_device=True)
    assert want["counts"].sum() > 0
    _same(got, want)
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_flag_within_lists_equal_match_within(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng)
    min_cos, cap = 0.02, 64
    eng.set_within(min_cos, cap)
    want = eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, nms_iou=0.4)
    got = eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, nms_iou=0.4, flags=native.FLAG_WITHIN, on_device=True)
    _same(got, want)
    idx, cos, n = eng.fetch_within()
    live = np.arange(K)[None, :] < got["counts"][:, None]
    assert idx.shape == (2, K, cap) and not n[~live].any() and n[live].min() > 0 and n.max() <= cap
    w_idx, w_cos, w_n = eng.match_within(got["emb"][live], min_cos, cap)
    assert np.array_equal(idx[live], w_idx) and np.array_equal(cos[live], w_cos) and np.array_equal(n[live], w_n)


def test_state_between_calls(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng)
    H, W = frames.shape[1:3]
    hws = [pyramid.scaled_size(H, W, s) for s in SCALES]
    eng.upload_frames(frames)
    eng.process_resident(max_faces=K, det_thresh=THR)
    plain = eng.fetch_results()
    # the same call twice: the same bits
    a = eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, on_device=True)
    b = eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, on_device=True)
    _same(a, b)
    second = eng.process_frames_pyramid(frames, SCALES[1:], max_faces=K, det_thresh=0.35, on_device=True)
    assert not np.array_equal(second["boxes"], a["boxes"])
    # two calls queued without a fetch in between: the fetch returns the second one's results, the counters see both
    eng.upload_frames(frames)
    eng.reset_counters()
    eng.process_pyramid_resident(hws, max_faces=K, det_thresh=THR)
    eng.process_pyramid_resident(hws[1:], max_faces=K, det_thresh=0.35)
    _same(eng.fetch_results(), second)
    ctr = eng.counters()
    assert ctr["faces"] == int(a["counts"].sum()) + int(second["counts"].sum()) and ctr["calls"] == 2 and ctr["frames"] == 4
    # the detector source stays at the last scale ...
    assert eng.det_source().shape[1:3] == hws[2]
    # ... and a plain pass switches back to full size by itself
    eng.process_resident(max_faces=K, det_thresh=THR)
    _same(eng.fetch_results(), plain)
    assert eng.det_source().shape[1:3] == (H, W)


def test_stage_timers_add_up():
    eng = native.Engine(0, profile=True)
    try:
        frames = _ready(eng)
        eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, on_device=True)
        eng.reset_counters()
        eng.upload_frames(frames)
        eng.process_pyramid_resident([pyramid.scaled_size(360, 500, s) for s in SCALES], max_faces=K, det_thresh=THR)
        eng.fetch_results()
        c = eng.counters()
        stages = sum(v for k, v in c.items() if k.startswith("ms_") and k != "ms_total")
        assert c["ms_total"] > 0 and abs(stages - c["ms_total"]) <= 1e-3 * c["ms_total"] + 1e-3      # (event times are fp32 milliseconds)
        assert c["ms_preprocess"] > c["ms_det_conv"]          # the earlier scales are counted there (frp.h)
    finally:
        eng.close()


def _refused(fn):
    with pytest.raises(FrpError) as e:
        fn()
    assert str(e.value).split(":", 1)[1].strip()          # "frp error <code>: <the library's message>"
    return e.value


def test_refusals_leave_the_handle_working(fresh_engine):
    eng = fresh_engine
    frames, G = _input()
    hws = [pyramid.scaled_size(360, 500, s) for s in SCALES]
    eng.upload_frames(frames)
    _refused(lambda: eng.process_pyramid_resident(hws, max_faces=K))                          # no weights
    bare = native.Engine(0)
    try:
        bare.load_weights(get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))[1])
        _refused(lambda: bare.process_pyramid_resident(hws, max_faces=K))                     # no resident frames
    finally:
        bare.close()
    _ready(eng)
    want = eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR)
    eng.upload_frames(frames)
    eng.process_pyramid_resident(hws, max_faces=K, det_thresh=THR)
    for bad in ([], hws + hws[:2]):                                                           # 0 and 5 scales
        _refused(lambda: eng.process_pyramid_resident(bad, max_faces=K))
    _refused(lambda: eng.process_pyramid_resident(hws + hws[:1], per_scale=129, max_faces=K))  # n_scales x per_scale > 512
    _refused(lambda: eng.process_pyramid_resident(hws, per_scale=0, max_faces=K))
    _refused(lambda: eng.process_pyramid_resident(hws, max_faces=129))
    _refused(lambda: eng.process_pyramid_resident([(0, 500)], max_faces=K))
    _refused(lambda: eng.process_pyramid_resident(hws, max_faces=K, flags=native.FLAG_FORCED_K))
    _refused(lambda: eng.process_pyramid_resident(hws, max_faces=K, flags=native.FLAG_WITHIN))   # frp_set_within never called
    # none of them overwrote the pass queued before them
    _same(eng.fetch_results(), want)
    eng._pass = (eng._pass[0], K // 2)                                                        # fetch_results with another K
    _refused(eng.fetch_results)
    eng._pass = (eng._pass[0], K)
    _same(eng.fetch_results(), want)
    # the debug entry: a count above per_scale, a NaN score on a live row (a dead row may hold anything)
    case = next(c for c in CASES if c["name"] == "exact_iou")
    args = lambda **kw: [kw.get(k, case[k]) for k in ("boxes", "kps", "scores", "counts")] + [case["K"], case["nms_iou"]]
    counts = case["counts"].copy()
    counts[1, 0] = case["scores"].shape[2] + 1
    _refused(lambda: eng.pyramid_merge(case["det_hws"], case["frame_hw"], *args(counts=counts)))
    counts[1, 0] = -1
    _refused(lambda: eng.pyramid_merge(case["det_hws"], case["frame_hw"], *args(counts=counts)))
    scores = case["scores"].copy()
    scores[0, 0, 1] = np.nan
    _refused(lambda: eng.pyramid_merge(case["det_hws"], case["frame_hw"], *args(scores=scores)))
    scores = case["scores"].copy()
    scores[0, 0, 3] = np.nan                                                                  # dead
    got = eng.pyramid_merge(case["det_hws"], case["frame_hw"], *args(scores=scores))
    assert all(np.array_equal(g, w) for g, w in zip(got, reference(case)))
    # ... and the debug entry touched nothing of the last pass; the handle still works
    _same(eng.fetch_results(), want)
    _same(eng.process_frames_pyramid(frames, SCALES, max_faces=K, det_thresh=THR, on_device=True), want)


def test_service_det_scales_on_the_real_engine(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng)
    eng.gallery_set(np.zeros((0, 512), np.float32))
    fs = FaceService(engine=eng)
    fs.ENCODINGS.clear()
    scales, thr = (1.0, 0.5), 0.30
    probe = eng.process_frames_pyramid(frames, scales, max_faces=10, det_thresh=thr, nms_iou=NMS_IOU, per_scale=PYRAMID_PER_SCALE,
                                       flags=native.FLAG_NO_MATCH)
    assert probe["counts"].min() >= 1
    rng = np.random.default_rng(5)
    for i in range(6):
        v = rng.standard_normal(512)
        assert fs.store_face(f"other{i}", v / np.linalg.norm(v))["success"]
    assert fs.store_face("first_of_frame0", probe["emb"][0, 0].astype(np.float64))["success"]
    want = eng.process_frames_pyramid(frames, scales, max_faces=10, det_thresh=thr, nms_iou=NMS_IOU, per_scale=PYRAMID_PER_SCALE)
    names = {int(r): fs.ENCODINGS.name_of_row(int(r)) for r in np.unique(want["match_idx"]) if r >= 0}
    got = fs.process_frames(frames, max_faces=10, det_thresh=thr, det_scales=scales)
    assert [len(f) for f in got] == want["counts"].tolist()
    for b, faces in enumerate(got):
        for k, face in enumerate(faces):
            assert face["bbox"] == want["boxes"][b, k].tolist() and face["kps"] == want["kps"][b, k].tolist()
            assert face["score"] == float(want["scores"][b, k]) and face["target"] == names[int(want["match_idx"][b, k])]
            assert np.array_equal(face["embedding"], want["emb"][b, k])
    assert got[0][0]["target"] == "first_of_frame0" and got[0][0]["match"]
    fs.ENCODINGS.clear()
