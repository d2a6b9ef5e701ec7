"""Face tracks without a GPU: tracks.TrackModel does on every case of tracks_cases what the case is named for (so the device tests,
which hold the kernels to the model on the same cases, reach every branch), the service and the mixer pass streams on or refuse, the
header declares what native.py binds, and the kernels use no scratch memory."""
import os
import re
import sys

import numpy as np
import pytest

from frp_amd import mixer, native, tracks
from frp_amd.face_service import FaceService, engine_caps

from fake_engine import FakeEngine
import tracks_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in tc.CASES}
f32 = np.float32


def _steps(name):
    """[(streams, boxes, counts, model output)] of the case's steps"""
    case = CASES[name]
    return [(op[1], op[2], op[3], o) for op, o in zip(case["ops"], tc.reference(case)) if op[0] == "step"]


def _live(counts, K):
    return np.arange(K)[None, :] < np.clip(counts, 0, K)[:, None]


def test_every_case_is_small_and_named_once():
    assert len(CASES) == len(tc.CASES) == 11
    for c in tc.CASES:
        for op in c["ops"]:
            if op[0] == "step":
                assert len(op[1]) <= 6 and (c["K"] <= 8 or c["name"] == "cut_at_T")
        assert sum(op[0] == "step" for op in c["ops"]) < 16          # stand_in's range


def test_stand_in_is_exact_and_distinct():
    e0, i0, c0 = tc.stand_in(3, 3, 128)
    e1, i1, c1 = tc.stand_in(4, 3, 128)
    assert e0.dtype == f32 and np.array_equal(e0.astype(np.float64), 3 * 2048 + np.arange(384)[:, None].reshape(3, 128, 1) + np.arange(512) / 512.0)
    assert len(np.unique(np.concatenate([e0[..., 0].ravel(), e1[..., 0].ravel()]))) == 768
    assert len(np.unique(np.concatenate([i0.ravel(), i1.ravel()]))) == 768 and len(np.unique(np.concatenate([c0.ravel(), c1.ravel()]))) == 768


def test_first_step_is_stale_and_the_empty_step_clears_it():
    m = tracks.TrackModel(max_streams=1)
    boxes = np.zeros((2, 2, 4), f32)
    boxes[:, 0] = (10, 10, 50, 60)
    o = m.step([0, 0], boxes, [1, 1], 2)
    assert o["reused"].sum() == 0 and o["track_id"][:, 0].tolist() == [0, 0] and o["n_embed"] == 2      # stale: the id continues, nothing reused
    o = m.step([0], boxes[:1], [1], 2)
    assert o["reused"][0, 0] == 1 and o["age"][0, 0] == 1


def test_batch_root():
    (_, _, _, o1), (_, _, _, o2) = _steps("batch_root")[1:]
    e, i, c = tc.stand_in(1, 3, 4)
    assert o1["reused"][:, :3].tolist() == [[0] * 3, [1] * 3, [1] * 3] and o1["n_embed"] == 3 and o1["face_slot"][:4].tolist() == [0, 1, 2, -1]
    for b in (1, 2):                      # frames 1 and 2 carry what frame 0 of the SAME batch computes
        assert np.array_equal(o1["emb"][b, :3], e[0, :3]) and np.array_equal(o1["idx"][b, :3], i[0, :3]) and np.array_equal(o1["cos"][b, :3], c[0, :3])
    assert o1["age"][:, 0].tolist() == [0, 1, 2] and o1["track_id"][:, :3].tolist() == [[0, 1, 2]] * 3
    assert o2["n_embed"] == 0 and np.array_equal(o2["emb"][1, :3], e[0, :3]) and o2["age"][:, 0].tolist() == [3, 4]      # ... out of the table


def test_two_streams_keep_their_own_state():
    steps = _steps("two_streams")[1:]
    assert steps[0][3]["track_id"].tolist() == [[0, 1, 2, -1], [0, 1, -1, -1]] * 2             # ids count per stream
    assert steps[0][3]["reused"].tolist() == [[0] * 4, [0] * 4, [1, 1, 1, 0], [1, 1, 0, 0]]
    for _, _, _, o in steps[1:]:
        assert o["n_embed"] == 0 and o["track_id"].tolist() == [[0, 1, 2, -1], [0, 1, -1, -1]] * 2
    assert steps[2][3]["age"][:, 0].tolist() == [4, 4, 5, 5]


def test_refresh_boundary():
    ages = np.concatenate([o["age"][:, 0] for _, _, _, o in _steps("refresh3")[1:]]).tolist()
    reused = np.concatenate([o["reused"][:, 0] for _, _, _, o in _steps("refresh3")[1:]]).tolist()
    assert ages == [0, 1, 2, 0, 1, 2, 0] and reused == [0, 1, 1, 0, 1, 1, 0]
    o = _steps("refresh3")[2][3]
    assert np.array_equal(o["emb"][1, 0], tc.stand_in(1, 4, 3)[0][3, 0])      # call 2, frame 1: embedded by call 1's LAST frame, not its first


def test_missed_faces_are_kept_max_missed_frames():
    (_, _, _, o1), (_, _, _, o2) = _steps("missed")[1:]
    assert o1["track_id"][0, :3].tolist() == [0, 1, 2]
    assert o2["track_id"][0, :2].tolist() == [0, 1] and o2["reused"][0, :2].tolist() == [1, 1] and o2["age"][0, 1] == 3       # absent 2 frames: back, reused
    assert np.array_equal(o2["emb"][0, 1], tc.stand_in(1, 3, 4)[0][0, 1])
    assert o2["track_id"][1, :3].tolist() == [0, 1, 3] and o2["reused"][1, 2] == 0                                           # absent 3 frames: a new id
    assert o2["reused"][2, :3].tolist() == [1, 1, 1]


def test_greedy_order_and_the_tie():
    _, boxes, _, o = _steps("greedy_tie")[1]
    e0, e1 = boxes[0, 0], boxes[0, 1]
    a, b = tracks.iou(boxes[1, 0], e0), tracks.iou(boxes[1, 0], e1)
    assert a.view(np.uint32) == b.view(np.uint32) and a == f32(0.6)                 # equal IoU BITS: the lower entry wins
    assert tracks.iou(boxes[1, 1], e0) > tracks.iou(boxes[1, 1], e1) >= f32(0.3)    # detection 1 would prefer entry 0: taken
    assert o["track_id"][1].tolist() == [0, 1, 2, 3] and o["reused"][1].tolist() == [1, 1, 1, 0]
    e = tc.stand_in(1, 2, 4)[0]
    assert np.array_equal(o["emb"][1, :3], e[0, :3]) and np.array_equal(o["emb"][1, 3], e[1, 3])


def test_at_and_just_below_iou_min():
    _, boxes, _, o = _steps("threshold")[1]
    assert tracks.iou(boxes[1, 0], boxes[0, 0]) == f32(0.5)
    below = tracks.iou(boxes[1, 1], boxes[0, 1])
    assert below < f32(0.5) and f32(0.5) - below <= f32(2.0 ** -24)                # two fp32 steps under the bound
    assert o["track_id"][1].tolist() == [0, 2] and o["reused"][1].tolist() == [1, 0]


def test_nan_iou_is_no_candidate():
    m = tracks.TrackModel(iou_min=0.01)
    inf = np.array([[[0, 0, np.inf, np.inf]]], f32)            # inf - inf in the union: NaN
    m.step([0], inf, [1], 1)
    assert np.isnan(tracks.iou(inf[0, 0], inf[0, 0]))
    o = m.step([0], inf, [1], 1)
    assert o["track_id"][0, 0] == 1 and o["reused"][0, 0] == 0


def test_empty_and_untracked_frames():
    steps = _steps("gaps")
    o = steps[1][3]
    assert o["track_id"].tolist() == [[0, 1, -1], [-1, -1, -1], [-1] * 3, [0, 1, -1], [-1, -1, -1], [0, 1, -1]]
    assert o["reused"].tolist() == [[0] * 3, [0] * 3, [0] * 3, [1, 1, 0], [0] * 3, [1, 1, 0]]
    assert o["age"][5, :2].tolist() == [3, 3] and o["n_embed"] == 5                    # the empty frame counted, the untracked ones did not
    assert steps[2][3]["n_embed"] == 1 and steps[2][3]["track_id"][0, 0] == -1
    assert steps[3][3]["track_id"][1, :2].tolist() == [1, 0] and steps[3][3]["reused"][1, :2].tolist() == [1, 1] and steps[3][3]["age"][1, 0] == 5


def test_the_cut_at_T_drops_entries():
    (_, _, _, o1), (_, _, _, o2) = _steps("cut_at_T")[1:]
    assert o1["track_id"][1, :100].tolist() == list(range(128, 228))
    assert o1["reused"][2].sum() == 28 and o1["reused"][2, :28].all()                  # 28 old entries survived the cut ...
    assert o1["track_id"][2, :28].tolist() == list(range(28)) and o1["track_id"][2, 28:].tolist() == list(range(228, 328))      # ... 100 fell out
    assert o2["n_embed"] == 0 and o2["reused"].sum() == 256
    assert len(tc.reference_model(CASES["cut_at_T"]).entries[0]) == tracks.TRACK_SLOTS


def test_stale_embeds_everything_once():
    steps = [o for _, _, _, o in _steps("stale")[1:]]
    assert steps[0]["reused"].tolist() == [[0] * 3, [1] * 3]
    assert steps[1]["reused"].sum() == 0 and steps[1]["track_id"].tolist() == [[0, 1, 2]] * 2 and steps[1]["age"].sum() == 0
    assert steps[2]["reused"].tolist() == [[1] * 3] and np.array_equal(steps[2]["emb"][0], tc.stand_in(2, 2, 3)[0][1])


def test_reset_of_one_stream():
    o = _steps("reset_one")[2][3]
    assert o["reused"].tolist() == [[0] * 3, [1, 1, 0], [1] * 3, [1, 1, 0]] and o["track_id"][0].tolist() == [0, 1, 2]
    assert o["age"][1, 0] == 1 and o["age"][0, 0] == 0


def test_a_batch_in_which_nothing_is_embedded():
    o = _steps("all_reused")[2][3]
    assert o["n_embed"] == 0 and (o["face_slot"] == -1).all() and o["reused"].sum() == 10


def test_the_cases_reuse_and_embed_at_least_a_third_each():
    live = reused = 0
    for c in tc.CASES:
        for op, o in zip(c["ops"], tc.reference(c)):
            if op[0] == "step":
                lv = _live(op[3], c["K"])
                live += int(lv.sum())
                reused += int(o["reused"][lv].sum())
                assert o["reused"][~lv].sum() == 0 and (o["track_id"][~lv] == -1).all() and not o["emb"][~lv].any()
    assert 3 * reused >= live and 3 * (live - reused) >= live, (live, reused)


def test_config_ranges():
    for bad in (dict(iou_min=0.0), dict(iou_min=1.5), dict(iou_min=float("nan")), dict(refresh=0), dict(max_missed=-1), dict(max_streams=0),
                dict(max_streams=65)):
        with pytest.raises(ValueError):
            tracks.TrackModel(**bad)
    with pytest.raises(ValueError):
        tracks.TrackModel(max_streams=2).step([2], np.zeros((1, 1, 4), f32), [0], 1)


# ------------------------------------------------------------------------------------------------ service and mixer
def test_frame_streams_and_run_mixed():
    meta = [("cam3", 0), ("cam7", 0), None, ("cam3", 1)]
    assert mixer.frame_streams(meta, ["cam3", "cam7"]) == [0, 1, -1, 0]

    class Service:
        seen = []

        def process_stream(self, batches, streams=None, **kw):
            for b in batches:
                self.seen.append((None if streams is None else list(streams(b)), kw))
                yield [[] for _ in range(len(b))]

    frames = np.zeros((3, 8, 8, 3), np.uint8)
    bufs = [np.zeros((4, 8, 8, 3), np.uint8) for _ in range(3)]
    mx = mixer.StreamMixer({"cam3": mixer.SyntheticStream(frames), "cam7": mixer.SyntheticStream(frames[:1])}, 4, bufs)
    svc = Service()
    list(mixer.run_mixed(svc, mx, track=True, max_faces=3))
    mx.close()
    assert [s[0] for s in svc.seen] == [[0, 1, 0, -1], [0, -1, -1, -1]] and svc.seen[0][1] == {"max_faces": 3}
    with pytest.raises(ValueError):
        list(mixer.run_mixed(svc, mx, groups_of_stream={}, track=True))


def test_an_engine_without_tracks_raises():
    eng = FakeEngine()
    assert not engine_caps(eng).track
    assert engine_caps(type("E", (), {m: None for m in ("track_config", "set_frame_streams", "fetch_tracks")})()).track
    svc = FaceService(engine=eng)
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="face tracks"):
        svc.process_frames(frames, streams=[0, 0])
    with pytest.raises(ValueError, match="face tracks"):
        svc.configure_tracks(2)
    with pytest.raises(ValueError, match="face tracks"):
        next(iter(svc.process_stream([frames], streams=[0, 0])))
    bufs = [np.zeros((2, 8, 8, 3), np.uint8) for _ in range(3)]
    mx = mixer.StreamMixer({"a": mixer.SyntheticStream(frames)}, 2, bufs)
    with pytest.raises(ValueError, match="face tracks"):
        list(mixer.run_mixed(svc, mx, track=True))
    mx.close()


def test_streams_refuse_what_they_do_not_combine_with():
    class TrackEngine(FakeEngine):
        def track_config(self, *a): pass
        def set_frame_streams(self, s): raise AssertionError("reached the engine")
        def fetch_tracks(self): pass

    svc = FaceService(engine=TrackEngine())
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    for kw in (dict(all_matches=True), dict(groups=[1, 1]), dict(det_scales=(1.0,))):
        with pytest.raises(ValueError, match="does not combine"):
            svc.process_frames(frames, streams=[0, 0], **kw)
    for bad in ([0], [0, -2], 5):
        with pytest.raises(ValueError, match="streams"):
            svc.process_frames(frames, streams=bad)


# ------------------------------------------------------------------------------------------------ the native side
def test_header_declares_what_native_binds():
    hdr = open(os.path.join(ROOT, "include", "frp.h")).read()
    lib = native.load_library()
    for name in ("frp_track_config", "frp_set_frame_streams", "frp_track_reset", "frp_fetch_tracks", "frp_track_stats", "frp_debug_track_step"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in native.ABI_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
    assert re.search(r"#define FRP_FLAG_TRACK 32u", hdr) and native.FLAG_TRACK == 32
    internal = open(os.path.join(ROOT, "face-recognition-platform_amd", "csrc", "frp_internal.h")).read()
    assert re.search(r"#define FRP_TRACK_SLOTS (\d+)", internal).group(1) == str(tracks.TRACK_SLOTS)
    assert re.search(r"#define FRP_TRACK_MAX_STREAMS (\d+)", hdr).group(1) == str(tracks.MAX_STREAMS)


def test_track_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    assert "-ffp-contract=off" in kernel_resources.makefile_flags("track_kernels")          # one rounding per operation, as the model
    kernels = kernel_resources.collect([("track_kernels", False)])["modules"]["track_kernels"]["kernels"]
    assert sorted(n.split("frp")[1][2:].split("kernel")[0] for n in kernels) == ["track_associate_", "track_compact_", "track_resolve_", "track_store_"]
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    assert "track_kernels" not in [m for m, _ in kernel_resources.GUARDED]
