"""CPU tests of the face-quality host side: FaceService.quality_from_sums (integer sums -> the reference's seven-key dict) against the
host method assess_face_quality, and the return_quality / quality keywords of the service on a test double of the engine."""
import json
import os
import re

import numpy as np

import quality_model
from fake_engine import FakeEngine
from frp_amd import native
from frp_amd.face_service import FaceService, box_to_location

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QUALITY_KEYS = ["score", "size_score", "position_score", "aspect_score", "blur_score", "lighting_score", "issues"]


def _cases():
    """(name, RGB image, location)"""
    rng = np.random.default_rng(20240607)
    out = []
    noise = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    for loc in ((0, 320, 240, 0), (17, 131, 90, 40), (100, 101, 240, 3), (239, 320, 240, 250)):
        out.append((f"noise{loc}", noise, loc))
    smooth = np.clip(128 + 40 * np.sin(np.arange(320) / 9.0)[None, :, None] + rng.normal(0, 3, size=(240, 320, 3)), 0, 255).astype(np.uint8)
    out.append(("smooth", smooth, (20, 300, 200, 30)))
    dark = rng.integers(0, 40, size=(97, 131, 3), dtype=np.uint8)
    out.append(("dark", dark, (3, 131, 97, 1)))
    yy, xx = np.mgrid[0:64, 0:64]
    cb = np.stack([(((yy + xx) % 2) * 255).astype(np.uint8)] * 3, -1)
    out.append(("checkerboard", cb, (0, 64, 64, 0)))
    out.append(("flat", np.full((64, 64, 3), 128, np.uint8), (0, 64, 64, 0)))
    out.append(("1x1", noise, (5, 8, 6, 7)))
    out.append(("1x17", noise, (9, 30, 10, 13)))
    out.append(("17x1", noise, (9, 14, 26, 13)))
    return out


def _unrounded(fs):
    q = fs._quality_history[-1]
    return [q["score"], q["blur_score"], q["lighting_score"]]


def test_quality_from_sums_equals_the_host_method():
    """sums from the numpy int64 model -> the dict of assess_face_quality on the same crop.  Unrounded scores to 1e-9 absolute: numpy's
    float64 var over the crop is not correctly rounded, the integer form is - the bound allows for the host's rounding, not ours."""
    host, dev = FaceService(engine=FakeEngine()), FaceService(engine=FakeEngine())
    for name, img, loc in _cases():
        want = host.assess_face_quality(img, loc)
        u_host = _unrounded(host)
        # on the host values alone: no score within 1e-6 of an x.xx5 rounding boundary (the seeds were chosen so)
        for v in u_host:
            assert abs((v * 100.0) % 1.0 - 0.5) > 1e-4, (name, v)
        top, right, bottom, left = loc
        s = quality_model.sums(img[None], (0, top, right, bottom, left), rgb=True)
        got = dev.quality_from_sums(img.shape, loc, (bottom - top) * (right - left), s)
        assert list(got.keys()) == QUALITY_KEYS
        for a, b in zip(_unrounded(dev), u_host):
            assert abs(a - b) <= 1e-9, (name, a, b)
        assert got == want, (name, got, want)
    assert len(dev._quality_history) == len(host._quality_history) == len(_cases())      # appended like the host method
    # the sums may pass 2^63 once multiplied by N: Python integers (a 4K checkerboard: N * L2 = 8.3e6 * 3.3e13)
    n = 3840 * 2160
    big = dev.quality_from_sums((2160, 3840, 3), (0, 3840, 2160, 0), n, [n // 2 * 255, n // 2 * 65025, 0, n * 2040 * 2040])
    assert big["blur_score"] == 100.0 and big["lighting_score"] == round((100.0 - 0.5 / 128 * 100 + 100.0) / 2, 2)


def test_quality_geometry_terms_of_the_reference_golden():
    meta = json.load(open(os.path.join(HERE, "golden", "plumbing_golden.json")))
    host, dev = FaceService(engine=FakeEngine()), FaceService(engine=FakeEngine())
    assert meta["quality"]
    n_dev = 0
    for q in meta["quality"]:
        shape, loc = tuple(q["shape"]), tuple(q["loc"])
        img = np.zeros(shape, np.uint8)
        top, right, bottom, left = loc
        got = host.assess_face_quality(img, loc)
        if 0 <= top < bottom <= shape[0] and 0 <= left < right <= shape[1]:        # a rectangle the device takes
            n_dev += 1
            assert dev.quality_from_sums(shape, loc, (bottom - top) * (right - left),
                                         quality_model.sums(img[None], (0, top, right, bottom, left), rgb=True)) == got
        for k in ("size_score", "position_score", "aspect_score"):
            assert got[k] == q["result"][k]
    assert n_dev >= 2


def test_tile_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "face-recognition-platform_amd", "csrc", "frp_internal.h")).read()
    th, tw = (int(re.search(rf"#define QUALITY_TILE_{d} (\d+)", hdr).group(1)) for d in "HW")
    assert (th, tw) == (native.QUALITY_TILE_H, native.QUALITY_TILE_W)
    assert "frp_face_quality" in native.ABI_SYMBOLS


class CountingEngine(FakeEngine):
    """FakeEngine that keeps the frames of its last pass, counts its passes and answers for any batch size; no face_quality"""

    def __init__(self):
        super().__init__()
        self.resident, self.passes = None, 0

    def process_frames(self, frames, **kw):
        self.resident = np.array(frames if frames.ndim == 4 else frames[None])
        self.passes += 1
        return _canned(self.resident.shape[0])


class QualityEngine(CountingEngine):
    """... with a numpy face_quality on those resident frames"""

    def __init__(self):
        super().__init__()
        self.quality_calls = []

    def face_quality(self, rects, rgb=False):
        rects = np.asarray(rects, np.int32).reshape(-1, 5)
        B, H, W, _ = self.resident.shape
        for f, top, right, bottom, left in rects.tolist():          # what frp_face_quality refuses must never arrive
            assert 0 <= f < B and 0 <= top < bottom <= H and 0 <= left < right <= W
        self.quality_calls.append((len(rects), rgb))
        return quality_model.sums_of(self.resident, rects, rgb)


BOXES = [[10.7, 20.2, 110.9, 140.1], [-5.0, 3.0, 700.0, 500.0], [700.0, 10.0, 720.0, 50.0], [0, 0, 0, 0]]   # third: empty after clipping
H, W, K = 480, 640, 4


def _canned(B, n_faces=3):
    emb = np.zeros((B, K, 512), np.float32)
    emb[:, 0, 0] = emb[:, 1, 1] = emb[:, 2, 2] = 1.0
    return dict(boxes=np.tile(np.array(BOXES, np.float32), (B, 1, 1)), kps=np.zeros((B, K, 5, 2), np.float32),
                scores=np.tile(np.array([0.9, 0.8, 0.7, 0], np.float32), (B, 1)), counts=np.full((B,), n_faces, np.int32), emb=emb,
                match_idx=np.full((B, K), -1, np.int32), match_cos=np.full((B, K), -1.0, np.float32))


def _image(seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


LOCS = [box_to_location(b, H, W) for b in BOXES[:3]]
ENCODE_KEYS = ["success", "face_count", "encodings", "message", "processing_time"]
FACE_KEYS = ["bbox", "kps", "score", "embedding", "target", "distance", "cosine", "confidence", "match"]


def _engines(B):
    plain = FakeEngine()
    plain.canned = _canned(B)
    return QualityEngine(), plain


def test_encode_face_return_quality_on_device_sums_and_on_the_fallback():
    img = _image(5)
    ref = FaceService(engine=FakeEngine())
    want = [ref.assess_face_quality(img, loc) for loc in LOCS]
    assert want[2]["blur_score"] == 50.0 and want[2]["lighting_score"] == 50.0           # the empty crop: the reference's default
    q, plain = _engines(1)
    for eng in (q, plain):
        fs = FaceService(engine=eng)
        r = fs.encode_face(img, return_locations=True, return_quality=True)
        assert list(r.keys()) == ENCODE_KEYS + ["locations", "quality"] and r["locations"] == LOCS
        assert r["quality"] == want and len(r["quality"]) == len(r["encodings"]) == 3
        assert len(fs._quality_history) == 3
        r = fs.encode_face(img, return_quality=True)
        assert list(r.keys()) == ENCODE_KEYS + ["quality"]
        # the defaults: exactly the keys of today, no quality work
        before = len(fs._quality_history)
        assert list(fs.encode_face(img).keys()) == ENCODE_KEYS
        assert list(fs.encode_face(img, return_locations=True).keys()) == ENCODE_KEYS + ["locations"]
        assert len(fs._quality_history) == before
    assert q.quality_calls == [(2, True), (2, True)]            # one call per image, the two rectangles the device takes, RGB order


def test_encode_cache_entry_without_quality_is_a_miss_when_quality_is_asked_for(tmp_path):
    from PIL import Image
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"img{i}.png"))
        Image.fromarray(_image(10 + i)).save(paths[-1])
    ref = FaceService(engine=FakeEngine())
    want = [[ref.assess_face_quality(_image(10 + i), loc) for loc in LOCS] for i in range(2)]
    for eng in (QualityEngine(), CountingEngine()):
        fs = FaceService(engine=eng)
        r = fs.encode_face(paths[0])
        assert list(r.keys()) == ENCODE_KEYS and eng.passes == 1
        r = fs.encode_face(paths[0], return_quality=True)                  # cached without quality: computed again
        assert "cached" not in r and eng.passes == 2 and r["quality"] == want[0]
        r = fs.encode_face(paths[0], return_quality=True)                  # the entry stored afterwards carries it
        assert r["cached"] is True and eng.passes == 2 and r["quality"] == want[0]
        r = fs.encode_face(paths[0])
        assert r["cached"] is True and "quality" not in r
        m = fs.get_performance_metrics()
        assert m["cache_hits"] == 2 and m["cache_misses"] == 2
        fs.clear_cache()
        fs.encode_face(paths[1])                                           # path 1 cached without quality, path 0 not cached
        rs = fs.batch_encode_faces(paths, return_quality=True)
        assert [r["quality"] for r in rs] == want and [r["image_path"] for r in rs] == paths
        assert not any("cached" in r for r in rs)
        rs = fs.batch_encode_faces(paths, return_quality=True)
        assert all(r["cached"] for r in rs) and [r["quality"] for r in rs] == want
        rs = fs.batch_encode_faces(paths)
        assert all("quality" not in r for r in rs)


def test_process_frames_quality_on_device_sums_and_on_the_fallback():
    frames = np.stack([_image(7), _image(8)])                  # BGR, as the camera loop delivers them
    ref = FaceService(engine=FakeEngine())
    want = [[ref.assess_face_quality(f[..., ::-1], loc) for loc in LOCS] for f in frames]
    q, plain = _engines(2)
    for eng in (q, plain):
        fs = FaceService(engine=eng)
        out = fs.process_frames(frames, max_faces=K, quality=True)
        assert [[f["quality"] for f in faces] for faces in out] == want
        assert all(list(f.keys()) == FACE_KEYS + ["quality"] for faces in out for f in faces)
        out = fs.process_frames(frames, max_faces=K, quality=True, all_matches=True)
        assert all(list(f.keys()) == FACE_KEYS + ["matches", "quality"] for faces in out for f in faces)
        before = len(fs._quality_history)
        out = fs.process_frames(frames, max_faces=K)               # the default: exactly the keys of today
        assert all(list(f.keys()) == FACE_KEYS for faces in out for f in faces) and len(fs._quality_history) == before
        assert all(list(f.keys()) == FACE_KEYS for f in fs.process_frame(frames[0]))
        streamed = list(fs.process_stream([frames, frames], max_faces=K, quality=True))
        assert [[[f["quality"] for f in faces] for faces in o] for o in streamed] == [want, want]
        assert all(list(f.keys()) == FACE_KEYS for o in fs.process_stream([frames], max_faces=K) for faces in o for f in faces)
    assert q.quality_calls == [(4, False)] * 4                 # one call per batch: the four rectangles the device takes, BGR order
