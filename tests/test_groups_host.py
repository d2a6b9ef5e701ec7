"""Gallery groups on the host (no GPU): the Gallery's mask table follows every update and reaches every copy, FaceService carries the
per-frame masks through its plan into the engine call sequence of every route, mixer.run_mixed builds them from a batch's meta, and
an engine that keeps no masks is never asked unless a mask is named.  The engine is a recording double defined here."""
import contextlib

import numpy as np
import pytest

from frp_amd import mixer, native, watchlist
from frp_amd.face_service import WITHIN_CAP, FaceService, engine_caps, within_min_cos
from frp_amd.gallery import GROUPS_ALL, Gallery
from frp_amd.yuv import YuvBatch, YuvFrame

from fake_engine import FakeEngine

f32 = np.float32
ALL = 0xFFFFFFFF
B, K, H, W = 2, 2, 48, 64


def _rows(n, seed=0):
    r = np.random.default_rng(seed).standard_normal((n, 512)).astype(f32)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


class GroupsEngine(FakeEngine):
    """FakeEngine + the row masks as the library keeps them (ALL for every row that arrives, moved by the swap-remove), recorded"""

    def __init__(self):
        super().__init__()
        self.masks = np.zeros(0, np.uint32)
        self.calls = []
        self.fail_remove = False

    def gallery_set(self, emb):
        super().gallery_set(np.asarray(emb))
        self.masks = np.full(len(self.G), ALL, np.uint32)
        self.calls.append(("gallery_set", len(self.G)))

    def gallery_update_row(self, row, emb):
        n = len(self.G)
        super().gallery_update_row(row, emb)
        if row == n:
            self.masks = np.concatenate([self.masks, np.array([ALL], np.uint32)])

    def gallery_remove_row(self, row):
        if self.fail_remove:
            self.fail_remove = False
            raise RuntimeError("device fault")
        super().gallery_remove_row(row)
        self.masks[row] = self.masks[-1]
        self.masks = self.masks[:-1].copy()

    def gallery_set_groups(self, groups, first=0):
        g = np.asarray(groups, np.uint32).reshape(-1)
        assert 0 <= first and first + len(g) <= len(self.G)
        self.masks[first:first + len(g)] = g
        self.calls.append(("gallery_set_groups", first, g.tolist()))

    def gallery_get_groups(self, first=0, n=None):
        return self.masks[first:(len(self.masks) if n is None else first + n)].copy()

    def set_frame_groups(self, masks):
        self.calls.append(("set_frame_groups", [int(m) for m in masks]))


def _agree(G, *engines):
    names = G.names()
    assert [G.name_of_row(i) for i in range(len(G))] == sorted(names, key=G.row_of)
    for e in engines:
        assert e.gallery_size() == len(G)
        assert np.array_equal(e.gallery_get_groups(), G.groups_table()), (e.gallery_get_groups(), G.groups_table())
    assert [G.groups_of(n) for n in names] == [int(G.groups_table()[G.row_of(n)]) for n in names]


# ------------------------------------------------------------------------------------------------ Gallery
def test_gallery_masks_follow_every_update_on_every_copy():
    main, mirror = GroupsEngine(), GroupsEngine()
    G = Gallery(lambda: main)
    G.add_mirror(mirror)
    R = _rows(8)
    assert G.put("a", R[0]) is False and G.groups_of("a") == GROUPS_ALL
    assert not any(c[0] == "gallery_set_groups" for c in main.calls + mirror.calls)       # a row without a mask: nobody is asked
    G.put("b", R[1], groups=0b0101)
    G.put("c", R[2], groups=0)                                       # enrolled, matches nobody
    G.put("d", R[3])
    _agree(G, main, mirror)
    assert [G.groups_of(n) for n in "abcd"] == [ALL, 0b0101, 0, ALL]
    assert G.put("b", R[4]) is True and G.groups_of("b") == 0b0101    # an overwrite keeps the mask ...
    assert G.put("b", R[4], groups=0b1000) is True and G.groups_of("b") == 0b1000         # ... unless one is named
    G.set_groups("d", 0b0011)
    _agree(G, main, mirror)
    assert G.remove("a")                                             # swap-remove: d (the last row) moves into row 0 with its mask
    assert G.row_of("d") == 0 and G.groups_of("d") == 0b0011 and G.names() == ["b", "c", "d"]
    _agree(G, main, mirror)
    assert G.remove("d") and G.remove("c")
    _agree(G, main, mirror)
    # set_bulk: one mask for all, one per row, none
    G.set_bulk(list("pqrs"), R[:4], groups=0b10)
    assert G.groups_table().tolist() == [0b10] * 4
    _agree(G, main, mirror)
    G.set_bulk(list("pqrs"), R[:4], groups=[1, 2, 4, ALL])
    assert G.groups_table().tolist() == [1, 2, 4, ALL]
    _agree(G, main, mirror)
    with pytest.raises(ValueError):
        G.set_bulk(list("pqrs"), R[:4], groups=[1, 2])
    main.calls.clear()
    G.set_bulk(list("pq"), R[:2])
    assert G.groups_table().tolist() == [ALL, ALL] and [c[0] for c in main.calls] == ["gallery_set"]
    _agree(G, main, mirror)
    # a removal that fails on the second copy: every copy is brought back to the table, masks included
    G.set_bulk(list("pqrs"), R[:4], groups=[1, 2, 4, 8])
    mirror.fail_remove = True
    with pytest.raises(RuntimeError):
        G.remove("p")
    assert G.names() == list("pqrs") and G.groups_table().tolist() == [1, 2, 4, 8]
    _agree(G, main, mirror)
    assert np.allclose(main.gallery_get(), mirror.gallery_get())
    G.clear()
    assert len(G) == 0 and len(G.groups_table()) == 0
    G.put("z", R[0], groups=3)
    _agree(G, main, mirror)


def test_an_engine_without_masks_is_only_asked_when_a_mask_is_named():
    eng = FakeEngine()                                               # no gallery_set_groups, no set_frame_groups
    assert not engine_caps(eng).groups and engine_caps(GroupsEngine()).groups
    G = Gallery(lambda: eng)
    R = _rows(4, 1)
    G.put("a", R[0])
    G.put("b", R[1], groups=ALL)                                     # ALL is what the row has anyway
    G.set_bulk(["a", "b", "c"], R[:3])
    G.set_bulk(["a", "b", "c"], R[:3], groups=ALL)
    G.remove("a")
    assert G.groups_table().tolist() == [ALL, ALL] and G.names() == ["b", "c"]
    before = eng.gallery_get().copy()
    for call in (lambda: G.put("d", R[3], groups=5), lambda: G.put("b", R[3], groups=5), lambda: G.set_groups("b", 1),
                 lambda: G.set_bulk(["x"], R[:1], groups=[4])):
        with pytest.raises(ValueError):
            call()
    assert G.names() == ["b", "c"] and np.array_equal(eng.gallery_get(), before)          # nothing was touched
    svc = FaceService(engine=FakeEngine())
    assert svc.store_face("a", R[0])["success"]
    with pytest.raises(ValueError):
        svc.process_frames(np.zeros((B, H, W, 3), np.uint8), groups=[1, 2])
    assert svc.store_face("m", R[1], groups=2)["success"] is False   # (store_face reports errors in its result, as the reference does)


def test_install_watchlist_passes_one_mask_for_the_list():
    eng = GroupsEngine()
    svc = FaceService(engine=eng)
    recs = [{"target": f"t{i}", "embedding": watchlist.encrypt_embedding(r.tolist(), None)} for i, r in enumerate(_rows(3, 2))]
    assert watchlist.install_watchlist(svc, recs, None, groups=0b100) == {"loaded": 3, "skipped": 0}
    assert eng.masks.tolist() == [0b100] * 3 and svc.ENCODINGS.groups_of("t1") == 0b100
    assert watchlist.install_watchlist(svc, recs, None) == {"loaded": 3, "skipped": 0}
    assert eng.masks.tolist() == [ALL] * 3


# ------------------------------------------------------------------------------------------------ FaceService: plan and call order
def _canned(n_frames=B):
    emb = np.zeros((n_frames, K, 512), f32)
    emb[:, :, 0] = 1.0
    return dict(boxes=np.tile(np.array([[2.0, 2.0, 20.0, 20.0]], f32), (n_frames, K, 1)), kps=np.zeros((n_frames, K, 5, 2), f32),
                scores=np.full((n_frames, K), 0.9, f32), counts=np.full(n_frames, 1, np.int32), emb=emb,
                match_idx=np.zeros((n_frames, K), np.int32), match_cos=np.full((n_frames, K), 0.99, f32))


class RouteEngine(GroupsEngine):
    """... + the blocking pass, the pyramid, the radius match of a pass and the staged / lane calls of native.Engine, recorded"""

    def sequence(self):
        return contextlib.nullcontext()

    def process_frames(self, frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_frames", flags))
        self._n = len(frames)
        return _canned(len(frames))

    def process_frames_pyramid(self, frames, scales=(1.0,), max_faces=10, det_thresh=0.5, nms_iou=0.4, per_scale=64, flags=0, on_device=False):
        self.calls.append(("process_frames_pyramid", flags))
        self._n = len(frames)
        return _canned(len(frames))

    def process_pyramid_resident(self, det_hws, per_scale=64, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_pyramid_resident", flags))

    def set_within(self, min_cos, cap=64):
        self.calls.append(("set_within", min_cos, cap))

    def fetch_within(self):
        self.calls.append(("fetch_within",))
        n = self._n
        return np.full((n, K, WITHIN_CAP), -1, np.int32), np.full((n, K, WITHIN_CAP), -2.0, f32), np.zeros((n, K), np.int32)

    _n = B

    def upload_frames_async(self, frames):
        self.calls.append(("upload_frames_async", len(frames)))
        self._staged = len(frames)

    def upload_yuv_async(self, batch):
        self.calls.append(("upload_yuv_async", len(batch)))
        self._staged = len(batch)

    def swap_frames(self):
        self.calls.append(("swap_frames",))
        self._n = self._staged

    def process_resident(self, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self.calls.append(("process_resident", flags))

    def fetch_results(self):
        self.calls.append(("fetch_results",))
        return _canned(self._n)


def _service(enrolled=True):
    eng = RouteEngine()
    svc = FaceService(engine=eng)
    if enrolled:
        for i, r in enumerate(_rows(3, 5)):
            assert svc.store_face(f"n{i}", r, groups=1 << i)["success"]
    eng.calls.clear()
    return svc, eng


def _array():
    return np.zeros((B, H, W, 3), np.uint8)


def _yuv():
    return YuvBatch([YuvFrame(np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8)) for _ in range(B)], "NV12", "BT601")


GF = native.FLAG_GROUPS
MASKS = [0b01, 0b10]


def _names(calls):
    return [c[0] for c in calls]


def test_plan_carries_the_masks_and_the_flag():
    svc, eng = _service()
    caps = engine_caps(eng)
    p = svc._plan(caps, True, K, None, None, False, False, None, (1, 2))
    assert p.groups == (1, 2) and p.flags == GF and not p.within
    p = svc._plan(caps, True, K, None, None, True, False, None, (1, 2))
    assert p.groups == (1, 2) and p.flags == GF | native.FLAG_WITHIN and p.within
    p = svc._plan(caps, False, K, None, None, True, False, None, (1, 2))          # empty gallery: no match, so no grouped match
    assert p.groups is None and p.flags == native.FLAG_NO_MATCH
    p = svc._plan(caps, True, K, None, None, False, False, None)
    assert p.groups is None and p.flags == 0


@pytest.mark.parametrize("all_matches", [False, True])
def test_every_route_sets_the_frame_masks_inside_the_pass_sequence(all_matches):
    arm = [("set_within", within_min_cos(0.6), WITHIN_CAP)] if all_matches else []
    fl = GF | (native.FLAG_WITHIN if all_matches else 0)
    tail = ["fetch_within"] if all_matches else []
    # blocking: one process call
    svc, eng = _service()
    svc.process_frames(_array(), max_faces=K, all_matches=all_matches, groups=MASKS)
    assert eng.calls == arm + [("set_frame_groups", MASKS), ("process_frames", fl)] + [(t,) for t in tail]
    # one int for all frames
    eng.calls.clear()
    svc.process_frames(_array(), max_faces=K, all_matches=all_matches, groups=0b100)
    assert eng.calls[len(arm)] == ("set_frame_groups", [0b100] * B)
    # blocking with det_scales: the pyramid call
    eng.calls.clear()
    svc.process_frames(_array(), max_faces=K, all_matches=all_matches, groups=MASKS, det_scales=(1.0, 0.5))
    assert eng.calls == arm + [("set_frame_groups", MASKS), ("process_frames_pyramid", fl)] + [(t,) for t in tail]
    # staged: upload, swap, pass, fetch
    eng.calls.clear()
    svc.process_frames(_yuv(), max_faces=K, all_matches=all_matches, groups=MASKS)
    assert eng.calls == arm + [("set_frame_groups", MASKS), ("upload_yuv_async", B), ("swap_frames",), ("process_resident", fl), ("fetch_results",)] + \
        [(t,) for t in tail]
    # overlapped (process_stream's lane form), masks per batch from a callable
    eng.calls.clear()
    batches = [_array(), _array()[:1]]
    per_batch = {id(batches[0]): MASKS, id(batches[1]): [0b11]}
    out = list(svc.process_stream(iter(batches), max_faces=K, all_matches=all_matches, groups=lambda b: per_batch[id(b)]))
    assert [len(o) for o in out] == [B, 1]
    sets = [c for c in eng.calls if c[0] == "set_frame_groups"]
    assert sets == [("set_frame_groups", MASKS), ("set_frame_groups", [0b11])]
    names = _names(eng.calls)
    for i, c in enumerate(eng.calls):
        if c[0] == "process_resident":
            assert c[1] == fl and "set_frame_groups" in names[:i] and names[i - 1] in ("set_frame_groups", "swap_frames")
    assert names.count("process_resident") == 2
    # without groups nothing of it appears, and an empty gallery never arms it
    eng.calls.clear()
    svc.process_frames(_array(), max_faces=K, all_matches=all_matches)
    assert "set_frame_groups" not in _names(eng.calls) and eng.calls[-1 - len(tail)][1] & GF == 0
    svc2, eng2 = _service(enrolled=False)
    svc2.process_frames(_array(), max_faces=K, all_matches=all_matches, groups=MASKS)
    assert eng2.calls == [("process_frames", native.FLAG_NO_MATCH)]
    # a wrong number of masks is refused before anything reaches the engine
    eng.calls.clear()
    for bad in ([1], [1, 2, 3], [1, 1 << 32]):
        with pytest.raises(ValueError):
            svc.process_frames(_array(), max_faces=K, groups=bad)
    assert eng.calls == []


def test_full_row_lists_honour_the_masks():
    """all_matches without the radius match: the score rows ignore groups, the service drops what the face's frame does not permit"""
    svc, eng = _service(enrolled=False)
    e = np.zeros(512, f32)
    e[0] = 1.0
    for name, mask in (("a", 0b01), ("b", 0b10), ("c", 0b11), ("d", 0)):
        assert svc.store_face(name, e, groups=mask)["success"]       # four identities on the canned face's own embedding
    svc.use_within = False
    out = svc.process_frames(_array(), max_faces=K, all_matches=True, groups=[0b01, 0b10])
    assert [m["target"] for m in out[0][0]["matches"]] == ["a", "c"]
    assert [m["target"] for m in out[1][0]["matches"]] == ["b", "c"]
    out = svc.process_frames(_array(), max_faces=K, all_matches=True)
    assert [m["target"] for m in out[0][0]["matches"]] == ["a", "b", "c", "d"]


# ------------------------------------------------------------------------------------------------ the mixer
def test_run_mixed_builds_the_frame_masks_from_the_meta():
    meta = [("cam3", 0), ("cam7", 0), None, ("cam9", 4)]
    assert mixer.frame_groups(meta, {"cam3": 0b001, "cam7": 0b101}) == [0b001, 0b101, 0, ALL]
    assert mixer.frame_groups(meta, lambda sid: 7 if sid == "cam9" else 1) == [1, 1, 0, 7]

    class Service:
        seen = []

        def process_stream(self, batches, groups=None, **kw):
            for b in batches:
                self.seen.append((None if groups is None else list(groups(b)), kw))
                yield [[] for _ in range(len(b))]

    frames = np.zeros((3, H, W, 3), np.uint8)
    streams = {"cam3": mixer.SyntheticStream(frames), "cam7": mixer.SyntheticStream(frames[:1])}          # cam7 ends after one frame
    bufs = [np.zeros((4, H, W, 3), np.uint8) for _ in range(3)]
    mx = mixer.StreamMixer(streams, 4, bufs)
    svc = Service()
    res = list(mixer.run_mixed(svc, mx, groups_of_stream={"cam3": 0b001, "cam7": 0b101}, max_faces=3))
    mx.close()
    assert [s[0] for s in svc.seen] == [[0b001, 0b101, 0b001, 0], [0b001, 0, 0, 0]] and svc.seen[0][1] == {"max_faces": 3}
    assert [sorted(r) for r in res] == [["cam3", "cam7"], ["cam3"]]
    svc.seen.clear()
    mx = mixer.StreamMixer({"cam3": mixer.SyntheticStream(frames)}, 4, bufs)
    list(mixer.run_mixed(svc, mx))
    mx.close()
    assert [s[0] for s in svc.seen] == [None]
