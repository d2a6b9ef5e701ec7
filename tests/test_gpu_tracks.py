"""Face tracks on the device (FRP_FLAG_TRACK; track_kernels.hip): the tracker's launches are held to tracks.TrackModel bit for bit
on every case of tracks_cases, a tracked pass to the model (who is embedded, who is reused, which id) and to UNTRACKED passes over
exactly the faces the model says are embedded - never to the tracked pass itself.

The network tests use blob (1, 2, 2, 2) / (1, 1, 1, 1) and at most 16 slots per call, so the tracked pass (launched for the capacity,
the count in device memory) and its untracked reference (launched for the count) stay in one embedder family, as in test_gpu_pyramid."""
import numpy as np
import pytest

from frp_amd import native, tracks
from frp_amd.face_service import FaceService
from frp_amd.native import FLAG_TRACK, FrpError

from conftest import get_raw_and_blob
from test_gpu_pyramid import _input
import tracks_cases as tc

pytestmark = pytest.mark.gpu

f32 = np.float32
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], f32) / f32(112)
STEP_KEYS = ("track_id", "reused", "age", "face_slot", "n_embed", "emb", "idx", "cos")
RES_KEYS = ("emb", "match_idx", "match_cos")


_PLANTED = []


def _proper_box_blob():
    """The seeded (1, 2, 2, 2) / (1, 1, 1, 1) weights predict NEGATIVE left + right distances on the seed-99 frames: every box the
    detector gives has x2 < x1.  Under the +1-pixel IoU of the NMS kernels such a box is empty - its IoU with anything, itself included,
    is 0 - so it never continues a track (test_inverted_boxes_match_nothing).  The tests that need the detector's faces to be found
    again use the same weights with the head's two x-distance rows negated, per anchor and level: the same logits, so the same
    anchors pass the threshold, and boxes with x1 < x2."""
    if not _PLANTED:
        from frp_amd import netspec, weights
        raw = dict(get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))[0])
        for lv in (3, 4, 5):
            for part in ("weight", "bias"):
                a = raw[f"det.head{lv}.out.{part}"].copy()
                for anchor in range(2):
                    for v in (1, 3):                    # left, right
                        a[anchor * netspec.DET_VALUES_PER_ANCHOR + v] *= -1
                raw[f"det.head{lv}.out.{part}"] = a
        _PLANTED.append(weights.pack_blob(raw, (1, 2, 2, 2), (1, 1, 1, 1)))
    return _PLANTED[0]


def _ready(eng, proper_boxes=False):
    frames, G = _input()
    eng.load_weights(_proper_box_blob() if proper_boxes else get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))[1])
    eng.gallery_set(G)
    eng.upload_frames(frames)
    return frames


def _face_list(frames, K):
    """per frame a list of boxes -> boxes [B, K, 4], kps [B, K, 5, 2] (the ArcFace template scaled into each box), scores, counts"""
    B = len(frames)
    boxes, kps = np.zeros((B, K, 4), f32), np.zeros((B, K, 5, 2), f32)
    scores, counts = np.zeros((B, K), f32), np.zeros((B,), np.int32)
    for b, rows in enumerate(frames):
        for k, box in enumerate(rows):
            boxes[b, k] = box
            kps[b, k] = boxes[b, k, :2] + TEMPLATE * (boxes[b, k, 2:] - boxes[b, k, :2])
            scores[b, k] = 0.9
        counts[b] = len(rows)
    return boxes, kps, scores, counts


def _live(counts, K):
    return np.arange(K)[None, :] < np.asarray(counts)[:, None]


# ------------------------------------------------------------------------------------------------ the launches alone
@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_track_step_equals_the_model(fresh_engine, case):
    eng = fresh_engine
    cfg = case["config"]
    eng.track_config(cfg["max_streams"], cfg["iou_min"], cfg["refresh"], cfg["max_missed"])
    call = 0
    for i, (op, want) in enumerate(zip(case["ops"], tc.reference(case))):
        if op[0] == "stale":
            eng.gallery_set(np.eye(1, 512, dtype=f32))               # any gallery mutation
        elif op[0] == "reset":
            eng.track_reset(op[1])
        else:
            _, streams, boxes, counts = op
            got = eng.track_step(streams, boxes, counts, case["K"], *tc.stand_in(call, len(streams), case["K"]))
            for k in STEP_KEYS:
                assert np.array_equal(got[k], want[k]), (case["name"], i, k)
            dead = ~_live(np.clip(counts, 0, case["K"]), case["K"])
            assert not got["emb"][dead].any() and (got["idx"][dead] == -1).all() and (got["cos"][dead] == -1).all()
            assert (got["track_id"][dead] == -1).all() and not got["reused"][dead].any() and not got["age"][dead].any()
            t = eng.fetch_tracks()
            assert all(np.array_equal(t[k], want[k]) for k in ("track_id", "reused", "age"))
            call += 1
    m = tc.reference_model(case)
    assert eng.track_stats() == (m.embedded, m.reused)


# ------------------------------------------------------------------------------------------------ a whole pass
K = 4
A, Bx, C, D, E = (60, 50, 140, 150), (250, 100, 330, 200), (100, 120, 180, 220), (300, 60, 380, 160), (400, 220, 470, 310)


def _sh(box, dx, dy=0):
    return (box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy)


# three calls on the two seed-99 frames, streams [0, 1]: boxes drift a few pixels; E appears in call 2 and D jumps beyond iou_min
MOTION = [[[A, Bx], [C, D]], [[_sh(A, 3, 1), _sh(Bx, -2, 2), E], [_sh(C, 2, 2), _sh(D, 0, 150)]],
          [[_sh(A, 5, 2), _sh(Bx, -4, 3), _sh(E, 1, 1)], [_sh(C, 4, 3), _sh(D, 2, 152)]]]
STREAMS = [0, 1]
_MOTION_RESULTS = {}


def _run_motion(eng, check_refs: bool):
    """the three tracked calls -> [(results, tracks)]; check_refs: every call is held to the model and to untracked passes"""
    _ready(eng)
    eng.track_config(2, 0.3, 8, 2)
    eng.set_frame_streams(STREAMS)
    model = tracks.TrackModel(0.3, 8, 2, 2)
    cache, outs = {}, []
    for call, frames in enumerate(MOTION):
        boxes, kps, scores, counts = _face_list(frames, K)
        got = eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK)
        trk = eng.fetch_tracks()
        outs.append((got, trk))
        if not check_refs:
            continue
        want = model.step(STREAMS, boxes, counts, K)
        for k in ("track_id", "reused", "age"):
            assert np.array_equal(trk[k], want[k]), (call, k)
        # the embedded slots: an UNTRACKED pass over exactly the model's embed list - same frames, same compact order, same count
        emb_slots = [[k for k in range(counts[b]) if not want["reused"][b, k]] for b in range(2)]
        assert [b * K + k for b in range(2) for k in emb_slots[b]] == want["face_slot"][:want["n_embed"]].tolist()
        if want["n_embed"]:
            rb, rk, rs, rc = _face_list([[frames[b][k] for k in emb_slots[b]] for b in range(2)], K)
            ref = eng.finish_faces(rb, rk, rs, rc, K)
            for b in range(2):
                for i, k in enumerate(emb_slots[b]):
                    for key in RES_KEYS:
                        assert np.array_equal(got[key][b, k], ref[key][b, i]), (call, b, k, key)
                    assert ref["match_idx"][b, i] >= 0
                    cache[(STREAMS[b], int(want["track_id"][b, k]))] = tuple(ref[key][b, i].copy() for key in RES_KEYS)
        # the reused slots: the bits the same track had in the call that embedded it
        for b in range(2):
            for k in range(counts[b]):
                if want["reused"][b, k]:
                    for key, v in zip(RES_KEYS, cache[(STREAMS[b], int(want["track_id"][b, k]))]):
                        assert np.array_equal(got[key][b, k], v), (call, b, k, key)
        dead = ~_live(counts, K)
        assert not got["emb"][dead].any() and (got["match_idx"][dead] == -1).all() and (got["match_cos"][dead] == -1).all()
    if check_refs:
        assert [int(t["reused"].sum()) for _, t in outs] == [0, 3, 5] and outs[1][1]["track_id"].tolist() == [[0, 1, 2, -1], [0, 2, -1, -1]]
        assert eng.track_stats() == (model.embedded, model.reused) == (6, 8)
        assert eng.counters()["faces"] == 6 + 6              # frp_counters.faces: embedded faces, of the tracked and the reference passes
    return outs


def _motion_default():
    if "default" not in _MOTION_RESULTS:
        eng = native.Engine(0)
        try:
            _MOTION_RESULTS["default"] = _run_motion(eng, check_refs=False)
        finally:
            eng.close()
    return _MOTION_RESULTS["default"]


def test_whole_pass_with_controlled_motion(fresh_engine):
    _MOTION_RESULTS["default"] = _run_motion(fresh_engine, check_refs=True)


def test_host_count_path_gives_the_same_bits(fresh_engine, monkeypatch):
    want = _motion_default()
    monkeypatch.setenv("FRP_HOST_COUNT", "1")
    got = _run_motion(fresh_engine, check_refs=True)           # (the references hold under the host count too)
    for call, ((g, gt), (w, wt)) in enumerate(zip(got, want)):
        for k in RES_KEYS:
            assert np.array_equal(g[k], w[k]), (call, k)
        for k in ("track_id", "reused", "age"):
            assert np.array_equal(gt[k], wt[k]), (call, k)


def test_stale_after_a_gallery_change(fresh_engine):
    eng = fresh_engine
    _ready(eng)
    eng.track_config(2)
    eng.set_frame_streams(STREAMS)
    boxes, kps, scores, counts = _face_list(MOTION[0], K)
    live = _live(counts, K)
    first = eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK)
    assert eng.track_stats() == (4, 0)
    again = eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK)                  # all reused: the cached bits, nothing embedded
    assert eng.track_stats() == (4, 4) and eng.fetch_tracks()["reused"][live].all()
    for key in RES_KEYS:
        assert np.array_equal(again[key], first[key]), key
    row = (int(first["match_idx"][0, 0]) + 1) % 64
    eng.gallery_update_row(row, first["emb"][0, 0])                                           # face (0, 0) now has a better row
    after = eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK)
    t = eng.fetch_tracks()
    assert eng.track_stats() == (8, 4) and not t["reused"].any() and t["track_id"][live].tolist() == [0, 1, 0, 1]
    ref = eng.finish_faces(boxes, kps, scores, counts, K)                                     # untracked, against the changed gallery
    for key in RES_KEYS:
        assert np.array_equal(after[key], ref[key]), key
    assert after["match_idx"][0, 0] == row != first["match_idx"][0, 0]
    assert np.array_equal(after["emb"], first["emb"])
    assert eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK) and eng.fetch_tracks()["reused"][live].all()      # ... and reuse resumes


def test_detector_in_front(fresh_engine):
    eng = fresh_engine
    _ready(eng, proper_boxes=True)
    Kd, thr = 8, 0.30
    eng.process_resident(max_faces=Kd, det_thresh=thr)
    want = eng.fetch_results()
    n = want["counts"]
    assert n.min() >= 2 and n.max() <= Kd
    live = _live(n, Kd)
    assert (want["boxes"][live][:, 2] > want["boxes"][live][:, 0]).all() and (want["boxes"][live][:, 3] > want["boxes"][live][:, 1]).all()
    eng.track_config(2, refresh=4)
    eng.set_frame_streams([0, 1])
    eng.process_resident(max_faces=Kd, det_thresh=thr, flags=FLAG_TRACK)
    one, t1 = eng.fetch_results(), eng.fetch_tracks()
    for k in want:
        assert np.array_equal(one[k], want[k]), k
    assert not t1["reused"].any() and all(t1["track_id"][b, :n[b]].tolist() == list(range(n[b])) for b in range(2))
    eng.process_resident(max_faces=Kd, det_thresh=thr, flags=FLAG_TRACK)
    two, t2 = eng.fetch_results(), eng.fetch_tracks()
    for k in want:
        assert np.array_equal(two[k], want[k]), k
    assert t2["reused"][live].all() and not t2["reused"][~live].any() and np.array_equal(t2["track_id"], t1["track_id"])
    assert (t2["age"][live] == 1).all() and eng.track_stats() == (int(n.sum()), int(n.sum()))
    # forced K: the count is known to the host, the tracked pass still runs from the device list
    eng.track_reset()
    eng.process_resident(max_faces=Kd, flags=native.FLAG_FORCED_K)
    forced = eng.fetch_results()
    for _ in range(2):
        eng.process_resident(max_faces=Kd, flags=native.FLAG_FORCED_K | FLAG_TRACK)
        got = eng.fetch_results()
        for k in forced:
            assert np.array_equal(got[k], forced[k]), k
    assert eng.fetch_tracks()["reused"].sum() > 0


def test_inverted_boxes_match_nothing(fresh_engine):
    """the seeded detector's boxes have x2 < x1 (_proper_box_blob): empty under the +1-pixel IoU, they continue no track - the second
    pass over the same frames gives every face a new id and embeds it, as the model says, and the results stay those of an untracked pass"""
    eng = fresh_engine
    _ready(eng)
    Kd, thr = 8, 0.30
    eng.process_resident(max_faces=Kd, det_thresh=thr)
    want = eng.fetch_results()
    live = _live(want["counts"], Kd)
    assert want["counts"].min() >= 2 and (want["boxes"][live][:, 2] < want["boxes"][live][:, 0]).all()
    eng.track_config(2, refresh=4)
    eng.set_frame_streams([0, 1])
    model = tracks.TrackModel(0.3, 4, 2, 2)
    for _ in range(2):
        eng.process_resident(max_faces=Kd, det_thresh=thr, flags=FLAG_TRACK)
        got, t, w = eng.fetch_results(), eng.fetch_tracks(), model.step([0, 1], want["boxes"], want["counts"], Kd)
        assert all(np.array_equal(t[k], w[k]) for k in ("track_id", "reused", "age")) and not t["reused"].any()
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    assert t["track_id"][0, 0] == want["counts"][0] and eng.track_stats() == (2 * int(want["counts"].sum()), 0)


def _refused(fn):
    with pytest.raises(FrpError) as e:
        fn()
    assert str(e.value).split(":", 1)[1].strip()
    return e.value


def test_refusals_leave_the_handle_and_the_tracks_alone(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng)
    boxes, kps, scores, counts = _face_list(MOTION[0], K)
    want = eng.finish_faces(boxes, kps, scores, counts, K)
    tracked = lambda **kw: eng.finish_faces(boxes, kps, scores, counts, K, flags=FLAG_TRACK | kw.get("flags", 0))
    _refused(tracked)                                                                # the flag without track_config
    _refused(lambda: eng.set_frame_streams([0, 1]))
    _refused(lambda: eng.track_config(65))
    _refused(lambda: eng.track_config(2, iou_min=0.0))
    _refused(lambda: eng.track_config(2, refresh=0))
    eng.track_config(2)
    _refused(tracked)                                                                # ... without set_frame_streams
    _refused(lambda: eng.set_frame_streams([0, 2]))                                  # a stream id >= max_streams
    _refused(tracked)
    eng.set_frame_streams([0, 1, 0])                                                 # another B
    _refused(tracked)
    _refused(lambda: eng.process_resident(max_faces=K, flags=FLAG_TRACK))
    _refused(lambda: eng.process_frames(frames, max_faces=K, flags=FLAG_TRACK))
    eng.set_frame_streams(STREAMS)
    eng.set_within(0.0, 8)
    eng.set_frame_groups([1, 1])
    _refused(lambda: tracked(flags=native.FLAG_WITHIN))
    _refused(lambda: tracked(flags=native.FLAG_GROUPS))
    _refused(lambda: eng.process_pyramid_resident([(360, 500)], max_faces=K, flags=FLAG_TRACK))
    _refused(lambda: eng.track_reset(2))
    _refused(lambda: eng.track_step([0, 3], boxes, counts, K, *tc.stand_in(0, 2, K)))
    # none of them overwrote the last pass, launched anything or advanced a track
    got = eng.fetch_results()
    for key in RES_KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert eng.track_stats() == (0, 0)
    model = tracks.TrackModel(max_streams=2)
    for _ in range(2):
        got, w = tracked(), model.step(STREAMS, boxes, counts, K)
        t = eng.fetch_tracks()
        assert all(np.array_equal(t[k], w[k]) for k in ("track_id", "reused", "age"))
        for key in RES_KEYS:
            assert np.array_equal(got[key], want[key]), key
    eng._track_pass = (2, K + 1)                                                     # fetch_tracks with another K
    _refused(eng.fetch_tracks)
    eng.track_config(0)                                                              # off: the flag is refused again
    _refused(tracked)


def test_service_process_frames_with_streams(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng, proper_boxes=True)
    eng.gallery_set(np.zeros((0, 512), f32))
    fs = FaceService(engine=eng)
    fs.ENCODINGS.clear()
    probe = eng.process_frames(frames, max_faces=8, det_thresh=0.30, flags=native.FLAG_NO_MATCH)
    rng = np.random.default_rng(5)
    for i in range(6):
        v = rng.standard_normal(512)
        assert fs.store_face(f"other{i}", v / np.linalg.norm(v))["success"]
    assert fs.store_face("first_of_frame0", probe["emb"][0, 0].astype(np.float64))["success"]
    with pytest.raises(FrpError):
        fs.process_frames(frames, max_faces=8, det_thresh=0.30, streams=[0, 1])               # configure_tracks first
    fs.configure_tracks(2)
    plain = fs.process_frames(frames, max_faces=8, det_thresh=0.30)
    one = fs.process_frames(frames, max_faces=8, det_thresh=0.30, streams=[0, 1])
    two = fs.process_frames(frames, max_faces=8, det_thresh=0.30, streams=[0, 1])
    assert [len(f) for f in one] == probe["counts"].tolist() == [len(f) for f in two]
    for b in range(2):
        for k, (p, a, c) in enumerate(zip(plain[b], one[b], two[b])):
            assert (a["track_id"], a["stream"], a["tracked"]) == (k, b, False) and (c["track_id"], c["stream"], c["tracked"]) == (k, b, True)
            for key in ("target", "distance", "cosine", "match", "bbox"):
                assert a[key] == p[key] == c[key], (b, k, key)
            assert np.array_equal(a["embedding"], p["embedding"]) and np.array_equal(c["embedding"], p["embedding"])
            assert "track_id" not in p
    assert one[0][0]["target"] == "first_of_frame0" and two[0][0]["match"]
    n = int(probe["counts"].sum())
    assert fs.track_statistics() == {"embedded": n, "reused": n}
    fs.reset_tracks(0)
    three = fs.process_frames(frames, max_faces=8, det_thresh=0.30, streams=[0, 1])
    assert [f["tracked"] for f in three[0]] == [False] * len(three[0]) and [f["tracked"] for f in three[1]] == [True] * len(three[1])
    streamed = list(fs.process_stream([frames, frames], max_faces=8, det_thresh=0.30, streams=lambda batch: [0, 1]))
    assert all(f["tracked"] for res in streamed for faces in res for f in faces)
    fs.ENCODINGS.clear()


@pytest.mark.selfcheck
def test_configured_but_unflagged_is_a_fresh_handle(fresh_engine):
    eng = fresh_engine
    frames = _ready(eng)
    eng.track_config(4, refresh=2)
    eng.set_frame_streams(STREAMS)
    eng.process_resident(max_faces=8, det_thresh=0.30, flags=FLAG_TRACK)
    eng.fetch_results()
    got = eng.process_frames(frames, max_faces=8, det_thresh=0.30)
    boxes, kps, scores, counts = _face_list(MOTION[0], K)
    got_ff = eng.finish_faces(boxes, kps, scores, counts, K)
    other = native.Engine(0)
    try:
        _ready(other)
        want = other.process_frames(frames, max_faces=8, det_thresh=0.30)
        want_ff = other.finish_faces(boxes, kps, scores, counts, K)
    finally:
        other.close()
    assert want["counts"].min() >= 2
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for k in RES_KEYS:
        assert np.array_equal(got_ff[k], want_ff[k]), k
