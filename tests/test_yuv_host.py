"""YUV 4:2:0 ingest, host side (no GPU): the contract's anchor pixels, the test model against its scalar form, yuv.to_bgr against the
model on every (Y, U, V) triple, strided planes and the four layouts, the ABI of the three new calls, and YuvBatch through the service
(fake engines: with and without the device path).  The device converter's turn is tests/test_gpu_yuv.py."""
import ctypes as C
import os
import re
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import quality_model  # noqa: E402
import yuv_model  # noqa: E402
from fake_engine import FakeEngine  # noqa: E402
from frp_amd import native, yuv  # noqa: E402
from frp_amd.face_service import FaceService  # noqa: E402


def test_anchor_pixels():
    for (Y, U, V), *want in yuv_model.ANCHORS:
        for matrix, bgr in zip(yuv_model.MATRICES, want):
            assert yuv_model.pixel(Y, U, V, matrix) == bgr, ((Y, U, V), matrix)
    # the literals once more, free of the table: grey stays grey, primaries saturate
    assert yuv_model.pixel(16, 128, 128, "BT601") == (0, 0, 0) and yuv_model.pixel(235, 128, 128, "BT709") == (255, 255, 255)
    assert yuv_model.pixel(81, 90, 240, "BT601") == (0, 0, 254) and yuv_model.pixel(81, 90, 240, "JFIF") == (14, 14, 238)
    assert yuv_model.pixel(200, 1, 254, "BT709") == (0, 174, 255) and yuv_model.pixel(0, 0, 0, "JFIF") == (0, 135, 0)


def _random_planes(rng, B, H, W, layout):
    Y = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    if layout in ("NV12", "NV21"):
        return Y, rng.integers(0, 256, (B, H // 2, W), dtype=np.uint8), None
    return Y, rng.integers(0, 256, (B, H // 2, W // 2), dtype=np.uint8), rng.integers(0, 256, (B, H // 2, W // 2), dtype=np.uint8)


@pytest.mark.parametrize("layout", yuv_model.LAYOUTS)
@pytest.mark.parametrize("matrix", yuv_model.MATRICES)
def test_model_frames_equal_the_scalar_form(layout, matrix):
    planes = _random_planes(np.random.default_rng(5), 3, 6, 10, layout)
    got = yuv_model.frames(planes, layout, matrix)
    Y, c1, c2 = planes
    for b in range(3):
        for y in range(6):
            for x in range(10):
                cy, cx = y >> 1, x >> 1
                if layout == "NV12":
                    U, V = c1[b, cy, 2 * cx], c1[b, cy, 2 * cx + 1]
                elif layout == "NV21":
                    V, U = c1[b, cy, 2 * cx], c1[b, cy, 2 * cx + 1]
                elif layout == "I420":
                    U, V = c1[b, cy, cx], c2[b, cy, cx]
                else:
                    V, U = c1[b, cy, cx], c2[b, cy, cx]
                assert tuple(got[b, y, x]) == yuv_model.pixel(Y[b, y, x], U, V, matrix), (b, y, x)
    assert np.array_equal(yuv.to_bgr(*planes, layout=layout, matrix=matrix), got)


def test_all_triples_holds_every_triple_once():
    Y, UV = yuv_model.all_triples()
    assert Y.shape == (4, 1024, 4096) and UV.shape == (4, 512, 4096)
    code = Y.astype(np.int64) | np.repeat(np.repeat(UV[..., 0::2], 2, 1), 2, 2).astype(np.int64) << 8 | np.repeat(np.repeat(UV[..., 1::2], 2, 1), 2, 2).astype(np.int64) << 16
    assert np.array_equal(np.bincount(code.ravel(), minlength=1 << 24), np.ones(1 << 24, np.int64))


@pytest.mark.parametrize("matrix", yuv_model.MATRICES)
def test_to_bgr_equals_the_model_on_every_triple(matrix):
    Y, UV = yuv_model.all_triples()
    assert np.array_equal(yuv.to_bgr(Y, UV, layout="NV12", matrix=matrix), yuv_model.triples_reference(matrix))


def test_strided_planes_and_the_four_layouts_agree():
    rng = np.random.default_rng(11)
    H, W = 12, 20
    Y, U, V = _random_planes(rng, 1, H, W, "I420")
    Y, U, V = Y[0], U[0], V[0]
    want = yuv_model.frames((Y[None], U[None], V[None]), "I420", "BT709")[0]
    UV, VU = np.stack([U, V], -1).reshape(H // 2, W), np.stack([V, U], -1).reshape(H // 2, W)
    for layout, c1, c2 in (("I420", U, V), ("YV12", V, U), ("NV12", UV, None), ("NV21", VU, None)):
        assert np.array_equal(yuv.to_bgr(Y, c1, c2, layout=layout, matrix="BT709"), want), layout
        # pitch > W and an odd pitch: views into wider buffers
        for pad in (12, 7):
            def wide(a):
                buf = rng.integers(0, 256, (a.shape[0], a.shape[1] + pad), dtype=np.uint8)
                buf[:, :a.shape[1]] = a
                return buf[:, :a.shape[1]]
            ys, c1s, c2s = wide(Y), wide(c1), None if c2 is None else wide(c2)
            assert ys.strides[0] == W + pad and not ys.flags.c_contiguous
            assert np.array_equal(yuv.to_bgr(ys, c1s, c2s, layout=layout, matrix="BT709"), want), (layout, pad)
            f = yuv.YuvFrame(ys, c1s, c2s)
            assert f.y_pitch == W + pad and f.c_pitch == c1.shape[1] + pad and f.y.ctypes.data == ys.ctypes.data      # taken as they lie
            batch = yuv.YuvBatch([f, f], layout, "BT709")
            assert batch.shape == (2, H, W, 3) and np.array_equal(batch.decode(), np.stack([want, want]))
            dev, yp, cp, table, _keep = batch.plane_table()
            assert (dev, yp, cp) == (False, W + pad, c1.shape[1] + pad) and table[0][0] == ys.ctypes.data and (table[0][2] == 0) == (c2 is None)
    # frames of unlike pitch in one batch: packed, one pitch pair
    a, b = yuv.YuvFrame(Y, UV), yuv.YuvFrame(wide(Y), wide(UV))
    dev, yp, cp, table, _keep = yuv.YuvBatch([a, b], "NV12").plane_table()
    assert (yp, cp) == (W, W) and len(table) == 2
    with pytest.raises(ValueError, match="even"):
        yuv.to_bgr(Y[:, :19], UV[:, :19])
    with pytest.raises(ValueError, match="layout"):
        yuv.to_bgr(Y, UV, layout="NV16")


NEW_SYMBOLS = ("frp_upload_yuv", "frp_upload_yuv_async", "frp_get_frames")


def test_abi_of_the_new_calls():
    lib = native.load_library()
    for name in NEW_SYMBOLS:
        assert name in native.ABI_SYMBOLS and hasattr(lib, name), name
    d = native.FrpYuvDesc(C.sizeof(native.FrpYuvDesc), 0, 0, 0, 4, 2, 4, 4)
    ptrs = (C.c_void_p * 3)()
    assert lib.frp_upload_yuv(None, C.byref(d), ptrs, 1) == -1
    assert lib.frp_upload_yuv_async(None, C.byref(d), ptrs, 1) == -1
    assert lib.frp_get_frames(None, None, 0, 0, 1) == -1
    assert native.YUV_LAYOUTS == {"NV12": 0, "NV21": 1, "I420": 2, "YV12": 3} and native.YUV_MATRICES == {"BT601": 0, "BT709": 1, "JFIF": 2}
    hdr = open(os.path.join(ROOT, "include", "frp.h")).read()
    for name, val in list(native.YUV_LAYOUTS.items()) + list(native.YUV_MATRICES.items()) + [("DEVICE", native.YUV_DEVICE)]:
        assert re.search(rf"#define FRP_YUV_{name} {val}\b", hdr), name


def test_desc_structure_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "frp.h")).read()
    body = re.search(r"typedef struct frp_yuv_desc \{(.*?)\} frp_yuv_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        size = 4 if ctype == "int32_t" else 8
        for n in names.split(","):
            off = (off + size - 1) // size * size          # natural alignment, as the C ABI lays plain integers out
            fields.append((n.strip(), off, size))
            off += size
    assert [f[0] for f in fields] == ["struct_size", "layout", "matrix", "flags", "width", "height", "y_pitch", "c_pitch"]
    assert C.sizeof(native.FrpYuvDesc) == (off + 7) // 8 * 8 == 40
    for n, o, size in fields:
        assert getattr(native.FrpYuvDesc, n).offset == o and getattr(native.FrpYuvDesc, n).size == size, n


# ------------------------------------------------------------------------------------------------- through the service

class _PixelEngine(FakeEngine):
    """a fake whose results are a function of the pixels it is handed: one face per frame, its box and embedding derived from the
    frame's content and matched against the fake gallery - any difference in the converted pixels shows in the results"""

    def process_frames(self, frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.ndim == 4
        B, K = len(frames), max_faces
        H, W = frames.shape[1:3]
        out = {"boxes": np.zeros((B, K, 4), np.float32), "kps": np.zeros((B, K, 5, 2), np.float32), "scores": np.zeros((B, K), np.float32),
               "counts": np.ones(B, np.int32), "emb": np.zeros((B, K, 512), np.float32),
               "match_idx": np.full((B, K), -1, np.int32), "match_cos": np.full((B, K), -2.0, np.float32)}
        for b, f in enumerate(frames):
            m = f.reshape(-1, 3).astype(np.float64).mean(0)
            x1, y1 = m[0] % (W - 24), m[1] % (H - 24)
            out["boxes"][b, 0] = [x1, y1, x1 + 20, y1 + 22]
            out["scores"][b, 0] = 0.9
            e = np.resize(f[::3, ::5].astype(np.float32).ravel() - 128.0, 512)
            out["emb"][b, 0] = e / np.linalg.norm(e)
            if len(self.G):
                i, c = self.match(out["emb"][b, 0][None])
                out["match_idx"][b, 0], out["match_cos"][b, 0] = i[0], c[0]
        return out


class _ResidentPixelEngine(_PixelEngine):
    """_PixelEngine that remembers the frames of its last pass and answers face_quality from them (the model of the device sums)"""

    def process_frames(self, frames, **kw):
        self.resident = np.asarray(frames)
        return super().process_frames(frames, **kw)

    def face_quality(self, rects, rgb=False):
        return quality_model.sums_of(self.resident, rects, rgb)


class _DeviceYuvEngine(_ResidentPixelEngine):
    """... with the staged-ingest surface of native.Engine, upload_yuv_async included (pixels from the test model)"""

    def __init__(self):
        super().__init__()
        self.calls = []
        self._seq = threading.RLock()

    def sequence(self):
        return self._seq

    def upload_yuv_async(self, batch):
        self.calls.append(("yuv", id(batch)))
        Y = np.stack([f.y for f in batch])
        c1 = np.stack([f.c1 for f in batch])
        c2 = None if batch[0].c2 is None else np.stack([f.c2 for f in batch])
        self.staged = yuv_model.frames((Y, c1, c2), batch.layout, batch.matrix)

    def upload_frames_async(self, frames):
        self.calls.append(("bgr", id(frames)))
        self.staged = np.asarray(frames)

    def swap_frames(self):
        self.resident = self.staged

    def process_resident(self, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        self._pass = dict(max_faces=max_faces, det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)

    def fetch_results(self):
        return _PixelEngine.process_frames(self, self.resident, **self._pass)


def _batches(n, B=3, hw=(48, 64), layout="NV12", matrix="BT601", seed=2):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        Y, c1, c2 = _random_planes(rng, B, hw[0], hw[1], layout)
        out.append(yuv.YuvBatch([yuv.YuvFrame(Y[b], c1[b], None if c2 is None else c2[b]) for b in range(B)], layout, matrix))
    return out


class _CountingBatch(yuv.YuvBatch):
    decodes = 0

    def decode(self):
        type(self).decodes += 1
        return super().decode()


def _service(eng):
    svc = FaceService(engine=eng)
    rng = np.random.default_rng(0)
    for i in range(5):
        svc.store_face(f"p{i}", rng.standard_normal(512))
    return svc


def _same_faces(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(x[k], y[k]) if isinstance(x[k], np.ndarray) else x[k] == y[k], k


@pytest.mark.parametrize("make_engine", [_ResidentPixelEngine, _DeviceYuvEngine])
@pytest.mark.parametrize("layout,matrix", [("NV12", "BT601"), ("I420", "BT709"), ("NV21", "JFIF"), ("YV12", "BT601")])
def test_service_results_for_a_yuv_batch_equal_those_for_its_pixels(make_engine, layout, matrix):
    batches = _batches(4, layout=layout, matrix=matrix)
    svc = _service(make_engine())
    for quality in (False, True):
        got = [svc.process_frames(b, max_faces=3, quality=quality) for b in batches]
        want = [svc.process_frames(b.decode(), max_faces=3, quality=quality) for b in batches]
        for g, w in zip(got, want):
            _same_faces(g, w)
            assert all(("quality" in f) == quality for faces in g for f in faces) and sum(len(f) for f in g) == 3
    got = list(svc.process_stream(iter(batches), max_faces=3, quality=True))
    want = list(svc.process_stream(iter([b.decode() for b in batches]), max_faces=3, quality=True))
    assert len(got) == 4
    for g, w in zip(got, want):
        _same_faces(g, w)
    # the pixels are the model's: the conversion is the contract, not merely self-consistent
    b0 = batches[0]
    model = yuv_model.frames((np.stack([f.y for f in b0]), np.stack([f.c1 for f in b0]), None if b0[0].c2 is None else np.stack([f.c2 for f in b0])), layout, matrix)
    assert np.array_equal(b0.decode(), model)


def test_an_engine_with_the_device_path_gets_the_surfaces_and_decode_is_never_called():
    eng = _DeviceYuvEngine()
    svc = _service(eng)
    batches = [_CountingBatch(list(b), b.layout, b.matrix) for b in _batches(5)]
    _CountingBatch.decodes = 0
    for b in batches[:2]:
        svc.process_frames(b, max_faces=3, quality=True)
    assert eng.calls == [("yuv", id(batches[0])), ("yuv", id(batches[1]))]
    eng.calls.clear()
    assert len(list(svc.process_stream(iter(batches), max_faces=3, quality=True))) == 5
    assert sorted(eng.calls) == sorted(("yuv", id(b)) for b in batches)          # once per batch, none as pixels
    assert _CountingBatch.decodes == 0
    # an engine without it: converted on the host, once per batch
    svc2 = _service(_ResidentPixelEngine())
    svc2.process_frames(batches[0], max_faces=3)
    assert _CountingBatch.decodes == 1


def test_odd_sizes_raise_before_any_engine_call():
    rng = np.random.default_rng(3)
    with pytest.raises(ValueError, match="even"):
        yuv.YuvBatch([yuv.YuvFrame(rng.integers(0, 256, (6, 9), dtype=np.uint8), rng.integers(0, 256, (3, 10), dtype=np.uint8))], "NV12")
    with pytest.raises(ValueError, match="even"):
        yuv.YuvBatch([yuv.YuvFrame(rng.integers(0, 256, (7, 10), dtype=np.uint8), rng.integers(0, 256, (3, 10), dtype=np.uint8))], "NV12")
    eng = _DeviceYuvEngine()
    svc = _service(eng)
    good = _batches(1)[0]
    good.hw = (47, 64)                                  # a batch that went bad after it was built
    with pytest.raises(ValueError, match="even"):
        svc.process_frames(good, max_faces=3)
    bad_frame = _batches(1)[0]
    bad_frame.append(yuv.YuvFrame(rng.integers(0, 256, (6, 10), dtype=np.uint8), rng.integers(0, 256, (3, 10), dtype=np.uint8)))
    with pytest.raises(ValueError, match="frame 3"):
        list(svc.process_stream(iter([bad_frame]), max_faces=3))
    assert eng.calls == []
    with pytest.raises(ValueError, match="two chroma planes"):
        yuv.YuvBatch(list(_batches(1)[0]), "I420")
    with pytest.raises(TypeError):
        yuv.YuvBatch([yuv.YuvFrame(4096, 8192, device=True, hw=(4, 4), y_pitch=256, c_pitch=256)], "NV12").decode()
