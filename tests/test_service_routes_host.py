"""FaceService's frame pass on a recording engine with canned, non-empty device results: which engine calls each route makes
and in what order (blocking: one process call; staged: upload, swap, pass, fetch; overlapped: process_stream's lane form), that the
three routes turn equal device results into equal result dicts, that "matches" is the reference's filter loop
(oracle/plumbing.py: camera_filter_loop) on the same distances whether the hit lists come from the radius match or from full score
rows, and what the metrics count.  Public surface only: process_frames, process_stream, process_frame, batch_compare_faces."""
import contextlib
import io
import threading

import numpy as np
import pytest

from frp_amd import native, pyramid
from frp_amd.face_service import DET_THRESH, NMS_IOU, PYRAMID_PER_SCALE, WITHIN_CAP, FaceService, box_to_location, cos_to_distance, within_min_cos
from frp_amd.mjpeg import JpegBatch, JpegFrame
from frp_amd.yuv import YuvBatch, YuvFrame
from oracle import plumbing

from fake_engine import FakeEngine

f32 = np.float32
B, K, H, W = 2, 4, 48, 64
COUNTS = [2, 1]
N_FACES = sum(COUNTS)
NAMES = ["ann", "bob", "cid", "dan", "eve"]
SCALES = (1.0, 0.5)
THRESHOLD = 0.5                                      # below the service tolerance (0.6): the bound is min(tolerance, threshold)
BOXES = [[4.2, 6.9, 30.1, 40.5], [33.0, 2.0, 60.7, 31.2], [10.0, 10.0, 20.0, 20.0], [0, 0, 0, 0]]        # inside the frame, not empty


def _directions():
    rng = np.random.default_rng(11)
    d = np.linalg.qr(rng.standard_normal((512, 6)))[0].T            # orthonormal rows
    return d


def _unit(v):
    return v / np.linalg.norm(v)


D = _directions()
# the three faces of the batch (frame 0: two, frame 1: one) and a five-row gallery around them: ann and eve are the same row (a
# tie the position decides), bob lies near face 0 (d ~ 0.3), cid near face 1 inside the bound (d ~ 0.45), dan near face 1 between
# THRESHOLD and the tolerance (d ~ 0.55: listed without threshold=, not with it); face 2 has nobody near it
FACES = np.stack([D[0], D[1], D[2]]).astype(f32)
GALLERY = np.stack([D[0], _unit(D[0] + 0.30 * D[3]), _unit(D[1] + 0.47 * D[4]), _unit(D[1] + 0.59 * D[5]), D[0]])


def _canned(n_frames=B, flags=0):
    """the device results of one pass over `n_frames` frames: counts [2, 1], K = 4, the top-1 of GALLERY planted (none under FLAG_NO_MATCH)"""
    emb = np.zeros((B, K, 512), f32)
    emb[0, 0], emb[0, 1], emb[1, 0] = FACES
    emb[0, 2:], emb[1, 1:] = 7.0, -7.0                                # dead slots hold junk nobody may read
    cos = (GALLERY @ FACES.T.astype(np.float64)).astype(f32)          # [5, 3]
    out = dict(boxes=np.tile(np.array(BOXES, f32), (B, 1, 1)), kps=np.arange(B * K * 10, dtype=f32).reshape(B, K, 5, 2),
               scores=np.tile(np.array([0.9, 0.8, 0.7, 0.6], f32), (B, 1)), counts=np.array(COUNTS, np.int32), emb=emb,
               match_idx=np.array([[0, 2, 3, 1], [-1, 4, 4, 4]], np.int32),
               match_cos=np.array([[cos[0, 0], cos[2, 1], 0.5, 0.5], [-1.0, 0.9, 0.9, 0.9]], f32))
    if flags & native.FLAG_NO_MATCH:
        out["match_idx"][:], out["match_cos"][:] = -1, -1.0
    return {k: v[:n_frames].copy() for k, v in out.items()}


class PlainEngine(FakeEngine):
    """records its hot-path calls; the blocking calls only (no staging, no device JPEG / YUV route), the pyramid pass, the radius
    match and face_quality.  `overflow`: the first face's hit list reports more hits than a list holds."""

    def __init__(self):
        super().__init__()
        self.calls = []
        self.overflow = False
        self.n_frames = B
        self.probe = lambda: None

    def sequence(self):
        return contextlib.nullcontext()

    def process_frames(self, frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.shape[1:] == (H, W, 3)
        self.calls.append(("process_frames", dict(max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        return _canned(len(frames), flags)

    def process_pyramid_resident(self, det_hws, per_scale=64, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_pyramid_resident", dict(det_hws=[tuple(hw) for hw in det_hws], per_scale=per_scale, max_faces=max_faces,
                                                            det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        self._flags = flags

    def process_frames_pyramid(self, frames, scales=(1.0, 0.5, 0.25), max_faces=10, det_thresh=0.5, nms_iou=0.4, per_scale=64, flags=0,
                               on_device=False):
        assert isinstance(frames, np.ndarray) and frames.shape[1:] == (H, W, 3)
        self.calls.append(("process_frames_pyramid", dict(scales=tuple(scales), max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou,
                                                          per_scale=per_scale, flags=flags, on_device=on_device)))
        return _canned(len(frames), flags)

    def match_scores(self, q):
        self.calls.append(("match_scores", len(q)))
        return FakeEngine.match_scores(self, q).astype(f32)          # float32, as the device returns them

    def match_within(self, q, min_cos, cap=64, record=True):
        if record:
            self.calls.append(("match_within", len(q), min_cos, cap))
        S = FakeEngine.match_scores(self, q).astype(f32)
        M = len(S)
        idx, cos, n = np.full((M, cap), -1, np.int32), np.full((M, cap), -2.0, f32), np.zeros(M, np.int32)
        for i in range(M):
            order = [j for j in np.argsort(-S[i].astype(np.float64), kind="stable") if S[i, j] >= f32(min_cos)]
            n[i] = len(order)
            idx[i, :len(order)], cos[i, :len(order)] = order, S[i, order]
        if self.overflow and M:
            n[0] = cap + 1                                            # the true count: the list was cut
        return idx, cos, n

    def set_within(self, min_cos, cap=64):
        self.calls.append(("set_within", min_cos, cap))
        self._within = (min_cos, cap)

    def fetch_within(self):
        self.calls.append(("fetch_within", None))
        min_cos, cap = self._within
        c = _canned(self.n_frames)
        nb = len(c["counts"])
        idx, cos, n = np.full((nb, K, cap), -1, np.int32), np.full((nb, K, cap), -2.0, f32), np.full((nb, K), 3 * cap, np.int32)   # dead slots: junk
        first = True
        for b in range(nb):
            k = int(c["counts"][b])
            idx[b, :k], cos[b, :k], n[b, :k] = self.match_within(c["emb"][b, :k], min_cos, cap, record=False)
            if not first:
                n[b, :k] = np.minimum(n[b, :k], cap)                  # (overflow is planted on the first face of the batch only)
            first = False
        return idx, cos, n

    def face_quality(self, rects, rgb=False):
        rects = np.asarray(rects, np.int64).reshape(-1, 5)
        self.calls.append(("face_quality", len(rects), rgb))
        return _sums(rects)


def _sums(rects):
    """planted device sums of rectangles (frame, top, right, bottom, left): a function of the rectangle alone"""
    n = (rects[:, 3] - rects[:, 1]) * (rects[:, 2] - rects[:, 4])
    return np.stack([100 * n, 10400 * n, 0 * n, (50 + 10 * rects[:, 0] + rects[:, 1]) * n], axis=1).astype(np.int64)


class StagedEngine(PlainEngine):
    """... with the staged-ingest calls of native.Engine, the device JPEG and YUV routes included.  `hold`: an event the first
    asynchronous pass waits for (the stream source sets it once the next batch has been delivered to the pipeline)."""

    def __init__(self):
        super().__init__()
        self.hold = None

    def _upload(self, name, batch):
        self.calls.append((name, len(batch)))
        self._staged_n = len(batch)

    def upload_frames_async(self, frames):
        assert isinstance(frames, np.ndarray)
        self._upload("upload_frames_async", frames)

    def upload_jpeg_async(self, jpegs):
        assert all(isinstance(j, bytes) for j in jpegs)
        self._upload("upload_jpeg_async", jpegs)

    def upload_yuv_async(self, batch):
        assert isinstance(batch, YuvBatch)
        self._upload("upload_yuv_async", batch)

    def swap_frames(self):
        self.calls.append(("swap_frames", None))
        self.n_frames = self._staged_n

    def _queued(self):
        if self.hold is not None:
            hold, self.hold = self.hold, None
            assert hold.wait(timeout=30)

    def process_resident(self, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_resident", dict(max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)))
        self._flags = flags
        self._queued()

    def process_pyramid_resident(self, *a, **kw):
        super().process_pyramid_resident(*a, **kw)
        self._queued()

    def fetch_results(self):
        self.calls.append(("fetch_results", self.probe()))
        return _canned(self.n_frames, self._flags)


# ------------------------------------------------------------------------------------------------------------- batches
def _array():
    return np.random.default_rng(3).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _jpeg():
    from PIL import Image
    frames = []
    for f in _array():
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=90)
        frames.append(JpegFrame(buf.getvalue()))
    return JpegBatch(frames, (H, W))


def _yuv():
    rng = np.random.default_rng(4)
    return YuvBatch([YuvFrame(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8))
                     for _ in range(B)], "NV12", "BT601")


MAKE = {"array": _array, "jpeg": _jpeg, "yuv": _yuv}
UPLOAD = {"array": "upload_frames_async", "jpeg": "upload_jpeg_async", "yuv": "upload_yuv_async"}
# (route, batch type, engine): an array is never staged by process_frames, and an engine without the device JPEG / YUV route gets
# a source batch decoded on the host through its blocking call
ROUTES = [("blocking", "array", PlainEngine), ("blocking", "jpeg", PlainEngine), ("blocking", "yuv", PlainEngine), ("blocking", "array", StagedEngine),
          ("staged", "jpeg", StagedEngine), ("staged", "yuv", StagedEngine),
          ("overlapped", "array", StagedEngine), ("overlapped", "jpeg", StagedEngine), ("overlapped", "yuv", StagedEngine)]
ALL_MATCHES = ["off", "within", "no_within", "overflow"]


@pytest.fixture(autouse=True)
def _setup(monkeypatch):
    monkeypatch.setenv("FRP_EXACT_COMPAT", "0")          # batch_compare_faces on cosines: the branch the radius match serves
    # the header of every frame of _jpeg() as the library's parser reports it (the device JPEG route asks per frame)
    monkeypatch.setattr(native, "jpeg_info", lambda data: {"width": W, "height": H, "components": 3, "h_samp": [2, 1, 1], "v_samp": [2, 1, 1],
                                                           "mcus_x": W // 16, "mcus_y": H // 16, "restart_interval": 0})


def _service(eng, enrolled):
    svc = FaceService(engine=eng)
    assert not svc.ENCODINGS.exact and svc.tolerance == 0.6
    if enrolled:
        for name, row in zip(NAMES, GALLERY):
            assert svc.store_face(name, row)["success"]
    eng.calls.clear()
    return svc


def _oracle_matches(eng, tolerance, threshold, monkeypatch):
    """per face the reference's filter loop on THE distances the service sees: cos_to_distance of the engine's float32 cosines"""
    o = plumbing.PlumbingOracle(tolerance)
    for name, row in zip(NAMES, GALLERY):
        o.ENCODINGS[name] = row.tolist()
    monkeypatch.setattr(plumbing, "face_distance", lambda stored, q: cos_to_distance(FakeEngine.match_scores(eng, np.asarray(q, f32))[0].astype(f32)))
    return [[{k: m[k] for k in ("target", "distance", "confidence")} for m in plumbing.camera_filter_loop(o, 0, [q], threshold)] for q in FACES]


def _expected_calls(route, kind, scales, am, quality, enrolled, n_batches=1):
    tol = THRESHOLD
    within = am in ("within", "overflow") and enrolled
    fl = (0 if enrolled else native.FLAG_NO_MATCH) | (native.FLAG_WITHIN if within else 0)
    common = dict(max_faces=K, det_thresh=DET_THRESH, nms_iou=NMS_IOU, flags=fl)
    arm = [("set_within", within_min_cos(tol), WITHIN_CAP)] if within else []
    after = [("face_quality", N_FACES, False)] if quality else []
    if am != "off" and enrolled:
        after += [("fetch_within", None)] if within else []
        after += [("match_scores", N_FACES)] if am in ("no_within", "overflow") else []
    if route == "blocking":
        one = ("process_frames", common) if scales is None else \
            ("process_frames_pyramid", dict(common, scales=scales, per_scale=PYRAMID_PER_SCALE, on_device=True))
        return arm + [one] + after
    run = ("process_resident", common) if scales is None else \
        ("process_pyramid_resident", dict(common, det_hws=[pyramid.scaled_size(H, W, s) for s in scales], per_scale=PYRAMID_PER_SCALE))
    up, swap = (UPLOAD[kind], B), ("swap_frames", None)
    if route == "staged":
        return arm + [up, swap, run, ("fetch_results", None)] + after
    calls = []
    for i in range(n_batches):            # the lane form: the next batch is staged under this one's kernels, ahead of the fetch, and
        calls += ([up] if i == 0 else []) + [swap] + arm + [run] + ([up] if i + 1 < n_batches else [])     # the previous batch's dicts
        calls += [("fetch_results", i * N_FACES)] + after                                                  # are built by then
    return calls


def _run(route, kind, make_engine, scales, am, quality, enrolled):
    """-> (service, engine, the result of every batch)"""
    eng = make_engine()
    eng.overflow = am == "overflow"
    svc = _service(eng, enrolled)
    svc.use_within = am != "no_within"
    kw = dict(max_faces=K, threshold=THRESHOLD, all_matches=am != "off", quality=quality, det_scales=scales)
    if route != "overlapped":
        return svc, eng, [svc.process_frames(MAKE[kind](), **kw)]
    eng.probe = lambda: svc.get_performance_metrics()["total_encodings"]
    eng.hold = delivered = threading.Event()

    def source():
        yield MAKE[kind]()
        yield MAKE[kind]()
        delivered.set()                   # asked for a third batch: the second one is in the pipeline's hands
    return svc, eng, list(svc.process_stream(source(), **kw))


def _same_result(got, want):
    assert len(got) == len(want)
    for fg, fw in zip(got, want):
        assert len(fg) == len(fw)
        for x, y in zip(fg, fw):
            assert list(x.keys()) == list(y.keys())
            for k in x:
                if k == "embedding":
                    assert np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype
                else:
                    assert x[k] == y[k] and type(x[k]) is type(y[k]), k


_BLOCKING = {}


def _blocking_result(scales, am, quality, enrolled):
    """what the plain blocking call on an array returns for these arguments: the result every route is compared with (computed once)"""
    key = (scales, am, quality, enrolled)
    if key not in _BLOCKING:
        _BLOCKING[key] = _run("blocking", "array", PlainEngine, scales, am, quality, enrolled)[2][0]
    return _BLOCKING[key]


@pytest.mark.parametrize("enrolled", [False, True], ids=["empty", "enrolled"])
@pytest.mark.parametrize("quality", [False, True], ids=["plain", "quality"])
@pytest.mark.parametrize("am", ALL_MATCHES)
@pytest.mark.parametrize("scales", [None, SCALES], ids=["native", "pyramid"])
@pytest.mark.parametrize("route,kind,make_engine", ROUTES, ids=[f"{r}-{k}-{e.__name__}" for r, k, e in ROUTES])
def test_calls_results_and_metrics_of_every_route(route, kind, make_engine, scales, am, quality, enrolled, monkeypatch):
    svc, eng, results = _run(route, kind, make_engine, scales, am, quality, enrolled)
    n_batches = 2 if route == "overlapped" else 1
    assert len(results) == n_batches
    assert eng.calls == _expected_calls(route, kind, scales, am, quality, enrolled, n_batches)
    m = svc.get_performance_metrics()
    assert m["total_encodings"] == n_batches * N_FACES
    assert m["total_comparisons"] == n_batches * N_FACES * (len(NAMES) if enrolled else 0)
    want = _blocking_result(scales, am, quality, enrolled)
    for got in results:
        _same_result(got, want)
    # ... and that result is the planted one
    got = results[0]
    assert [len(f) for f in got] == COUNTS
    faces = [f for frame in got for f in frame]
    keys = ["bbox", "kps", "score", "embedding", "target", "distance", "cosine", "confidence", "match"]
    assert all(list(f.keys()) == keys + (["matches"] if am != "off" else []) + (["quality"] if quality else []) for f in faces)
    c = _canned()
    for i, (b, k) in enumerate([(0, 0), (0, 1), (1, 0)]):
        f = faces[i]
        assert np.array_equal(f["embedding"], FACES[i]) and f["bbox"] == c["boxes"][b, k].tolist() and f["kps"] == c["kps"][b, k].tolist()
        assert f["score"] == float(c["scores"][b, k])
    if enrolled:
        d1 = float(cos_to_distance(c["match_cos"][0, 1]))
        assert [f["target"] for f in faces] == ["ann", "cid", None] and [f["match"] for f in faces] == [True, True, False]
        assert faces[0]["distance"] == float(cos_to_distance(c["match_cos"][0, 0])) and faces[0]["confidence"] == "high"
        assert faces[1]["distance"] == d1 and 0.4 < d1 < THRESHOLD and faces[1]["confidence"] == "medium"
        assert faces[1]["cosine"] == float(c["match_cos"][0, 1]) and faces[2]["distance"] is None and faces[2]["cosine"] is None
    else:
        assert all(f["target"] is None and f["match"] is False for f in faces)
    if am != "off":
        want_m = _oracle_matches(eng, svc.tolerance, THRESHOLD, monkeypatch) if enrolled else [[], [], []]
        assert [f["matches"] for f in faces] == want_m
        if enrolled:
            assert [[h["target"] for h in f["matches"]] for f in faces] == [["ann", "eve", "bob"], ["cid"], []]
    if quality:
        ref = FaceService(engine=FakeEngine())
        for i, (b, k) in enumerate([(0, 0), (0, 1), (1, 0)]):
            loc = box_to_location(BOXES[k], H, W)
            rect = np.array([[b, *loc]], np.int64)
            assert faces[i]["quality"] == ref.quality_from_sums((H, W, 3), loc, (loc[2] - loc[0]) * (loc[1] - loc[3]), _sums(rect)[0])


def test_the_threshold_only_narrows_the_tolerance(monkeypatch):
    eng = PlainEngine()
    svc = _service(eng, True)
    for threshold, tol in ((None, 0.6), (0.9, 0.6), (THRESHOLD, THRESHOLD)):
        for use_within in (True, False):
            svc.use_within = use_within
            eng.calls.clear()
            out = svc.process_frames(_array(), max_faces=K, threshold=threshold, all_matches=True)
            faces = [f for frame in out for f in frame]
            assert [f["matches"] for f in faces] == _oracle_matches(eng, 0.6, tol, monkeypatch)
            assert [h["target"] for h in faces[1]["matches"]] == (["cid", "dan"] if tol == 0.6 else ["cid"])
            if use_within:
                assert eng.calls[0] == ("set_within", within_min_cos(tol), WITHIN_CAP)


@pytest.mark.parametrize("scales", [None, (0.5,)], ids=["native", "pyramid"])
def test_process_frame_is_process_frames_of_one_frame(scales):
    eng = PlainEngine()
    svc = _service(eng, True)
    frame = _array()[0]
    meta = {"max_faces": K, "confidence_threshold": THRESHOLD, "det_scales": scales}
    got = svc.process_frame(frame, metadata=meta)
    common = dict(max_faces=K, det_thresh=DET_THRESH, nms_iou=NMS_IOU, flags=0)
    assert eng.calls == [("process_frames", common) if scales is None else
                         ("process_frames_pyramid", dict(common, scales=scales, per_scale=PYRAMID_PER_SCALE, on_device=True))]
    _same_result([got], svc.process_frames(frame[None], max_faces=K, threshold=THRESHOLD, det_scales=scales))
    assert [f["target"] for f in got] == ["ann", "cid"] and all("matches" not in f and "quality" not in f for f in got)
    assert svc.get_performance_metrics()["total_encodings"] == 2 * COUNTS[0]
    eng.calls.clear()
    assert len(svc.process_frame(frame)) == COUNTS[0] and eng.calls[0][1]["max_faces"] == 10


@pytest.mark.parametrize("mode", ["within", "no_within", "overflow"])
def test_batch_compare_faces_lists_what_the_reference_lists(mode, monkeypatch):
    eng = PlainEngine()
    eng.overflow = mode == "overflow"
    svc = _service(eng, True)
    svc.use_within = mode != "no_within"
    o = plumbing.PlumbingOracle(svc.tolerance)
    for name, row in zip(NAMES, GALLERY):
        o.ENCODINGS[name] = row.tolist()

    def distances(stored, q):                            # the service's distances, in the order of the oracle's target list
        rows = [next(i for i, r in enumerate(GALLERY) if np.array_equal(r, s)) for s in np.asarray(stored)]
        return cos_to_distance(FakeEngine.match_scores(eng, np.asarray(q, f32))[0].astype(f32))[rows]
    monkeypatch.setattr(plumbing, "face_distance", distances)
    queries = list(FACES)
    listed = [("match_within", len(queries), within_min_cos(svc.tolerance), WITHIN_CAP)] if mode != "no_within" else []
    rows = [("match_scores", len(queries))] if mode != "within" else []
    for names in (None, ["dan", "nobody", "bob", "cid"]):
        eng.calls.clear()
        got = svc.batch_compare_faces(queries, target_names=names)
        want = o.batch_compare_faces(queries, target_names=names)
        assert got == want and eng.calls == listed + rows
        assert all(list(m.keys()) == ["target", "match", "distance", "confidence"] and m["match"] is True and type(m["distance"]) is float
                   for r in got for m in r)
    assert [[m["target"] for m in r] for r in svc.batch_compare_faces(queries)] == [["ann", "eve", "bob"], ["cid", "dan"], []]
    # eve listed twice has two positions (ann is the same row: the tie then goes by position in the list): the full rows, whatever the mode
    eng.calls.clear()
    twice = svc.batch_compare_faces(queries[:1], target_names=["eve", "ann", "eve"])
    assert [m["target"] for m in twice[0]] == ["eve", "ann", "eve"] and eng.calls == [("match_scores", 1)]
    assert svc.batch_compare_faces([], target_names=None) == [] and svc.batch_compare_faces(queries, target_names=["nobody"]) == [[], [], []]
