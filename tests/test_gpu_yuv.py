"""GPU: YUV 4:2:0 surfaces -> resident BGR frames (frp_upload_yuv / frp_upload_yuv_async, csrc/yuv_kernels.hip), read back through
frp_get_frames and compared byte for byte with tests/yuv_model.py.  Host planes are packed into a device staging buffer before the
kernel runs, so what the fast path asks of pitches and addresses is exercised with DEVICE surfaces (a torch tensor laid out the way
a decoder's pool would be); every shape runs from both kinds of source."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch       # (before the first engine: the process then runs on ONE HIP runtime, as in the other GPU test files)

import yuv_model
from conftest import get_raw_and_blob
from frp_amd import native, yuv
from frp_amd.face_service import FaceService

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SEMI = ("NV12", "NV21")


def _planes(rng, B, H, W, layout):
    Y = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    if layout in SEMI:
        return Y, rng.integers(0, 256, (B, H // 2, W), dtype=np.uint8), None
    return Y, rng.integers(0, 256, (B, H // 2, W // 2), dtype=np.uint8), rng.integers(0, 256, (B, H // 2, W // 2), dtype=np.uint8)


def _pool(planes, y_pitch=None, c_pitch=None, gap_rows=0, reverse=False, shift=()):
    """the surfaces of a batch inside ONE byte buffer full of noise, as a decoder's pool holds them: per frame the Y rows at y_pitch,
    `gap_rows` rows of padding, the chroma plane(s) at c_pitch, every plane on a 256-byte boundary; `reverse`: frame 0 at the highest
    address; `shift`: frames whose Y plane starts one byte later.  -> (u8 buffer, [[y, c1, c2 offsets]], y_pitch, c_pitch)"""
    Y, c1, c2 = planes
    B, H, W = Y.shape
    y_pitch, c_pitch = y_pitch or W, c_pitch or c1.shape[2]
    up = lambda n: (n + 255) // 256 * 256       # noqa: E731
    o_c1 = up((H + gap_rows) * y_pitch + 1)
    o_c2 = up(o_c1 + c1.shape[1] * c_pitch)
    slot = up(o_c2 + (0 if c2 is None else c2.shape[1] * c_pitch))
    buf = np.random.default_rng(99).integers(0, 256, B * slot + 256, dtype=np.uint8)
    offs = []
    for b in range(B):
        base = ((B - 1 - b) if reverse else b) * slot
        oy = base + (1 if b in shift else 0)
        offs.append([oy, base + o_c1, 0 if c2 is None else base + o_c2])
        for plane, off, pitch in ((Y[b], oy, y_pitch), (c1[b], base + o_c1, c_pitch)) + (() if c2 is None else ((c2[b], base + o_c2, c_pitch),)):
            rows, width = plane.shape
            np.lib.stride_tricks.as_strided(buf[off:], (rows, width), (pitch, 1))[:] = plane
    return buf, offs, y_pitch, c_pitch


def _host_batch(planes, layout, matrix, **kw):
    buf, offs, yp, cp = _pool(planes, **kw)
    Y, c1, c2 = planes
    view = lambda off, shape, pitch: np.lib.stride_tricks.as_strided(buf[off:], shape, (pitch, 1))      # noqa: E731
    frames = [yuv.YuvFrame(view(o[0], Y.shape[1:], yp), view(o[1], c1.shape[1:], cp), None if c2 is None else view(o[2], c2.shape[1:], cp)) for o in offs]
    return yuv.YuvBatch(frames, layout, matrix), buf


def _device_batch(planes, layout, matrix, **kw):
    buf, offs, yp, cp = _pool(planes, **kw)
    t = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()                    # the surfaces are complete before the call (frp.h)
    base = t.data_ptr()
    assert base % 256 == 0
    H, W = planes[0].shape[1:]
    frames = [yuv.YuvFrame(base + o[0], base + o[1], None if planes[2] is None else base + o[2], device=True, hw=(H, W), y_pitch=yp, c_pitch=cp) for o in offs]
    return yuv.YuvBatch(frames, layout, matrix), t


_MAKE = {"host": _host_batch, "device": _device_batch}

# B, H, W, pool layout: the smallest shape of every path (fast: W % 16 == 0 and every plane and pitch aligned; else general)
SHAPES = {
    "2x2": (3, 2, 2, {}),
    "6x10_frame_stride": (3, 6, 10, {}),
    "2x16_fast_min": (2, 2, 16, {}),
    "4x32_fast": (2, 4, 32, {}),
    "4x18_past_a_strip": (2, 4, 18, {}),
    "4x34_past_two_strips": (2, 4, 34, {}),
    "34x48_pitch64": (2, 34, 48, dict(y_pitch=64, c_pitch=64)),
    "34x48_pitch50_49": (2, 34, 48, dict(y_pitch=50, c_pitch=49)),
    "4x32_second_frame_off_by_one": (2, 4, 32, dict(shift=(1,))),
}


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("layout", ["NV12", "I420"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_smallest_shapes_of_every_path(engine, shape, layout, source):
    B, H, W, kw = SHAPES[shape]
    planes = _planes(np.random.default_rng(7), B, H, W, layout)
    want = yuv_model.frames(planes, layout, "BT601")
    batch, keep = _MAKE[source](planes, layout, "BT601", **kw)
    engine.upload_yuv(batch)
    assert np.array_equal(engine.get_frames(), want)
    engine.upload_yuv_async(batch)
    engine.swap_frames()
    assert np.array_equal(engine.get_frames(), want)
    del keep


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("hw", [(6, 10), (4, 32)])
@pytest.mark.parametrize("layout,matrix", [("NV21", "BT601"), ("YV12", "BT601"), ("NV12", "BT709"), ("NV12", "JFIF"), ("I420", "BT709"), ("I420", "JFIF")])
def test_layouts_and_matrices(engine, layout, matrix, hw, source):
    planes = _planes(np.random.default_rng(8), 2, hw[0], hw[1], layout)
    batch, keep = _MAKE[source](planes, layout, matrix)
    engine.upload_yuv(batch)
    assert np.array_equal(engine.get_frames(), yuv_model.frames(planes, layout, matrix))
    del keep


def test_anchor_pixels_on_the_device(engine):
    A = yuv_model.ANCHORS
    n = len(A)
    Y = np.zeros((1, 2, 2 * n), np.uint8)
    UV = np.zeros((1, 1, 2 * n), np.uint8)
    for i, ((y, u, v), *_rest) in enumerate(A):
        Y[0, :, 2 * i:2 * i + 2] = y
        UV[0, 0, 2 * i], UV[0, 0, 2 * i + 1] = u, v
    for m, matrix in enumerate(yuv_model.MATRICES):
        engine.upload_yuv(_host_batch((Y, UV, None), "NV12", matrix)[0])
        got = engine.get_frames()[0]
        for i, a in enumerate(A):
            assert all(tuple(px) == a[1 + m] for px in got[:, 2 * i:2 * i + 2].reshape(-1, 3)), (a[0], matrix)


@pytest.mark.parametrize("matrix", yuv_model.MATRICES)
def test_every_triple_on_the_device(engine, matrix):
    """all 2^24 (Y, U, V) triples through the fast path (four 1024 x 4096 NV12 frames), then through the general path: the same
    frames two pixels wider - 4098 is no multiple of 16 -, the reference of the extra columns computed on their own"""
    Y, UV = yuv_model.all_triples()
    want = yuv_model.triples_reference(matrix)
    as_batch = lambda y, c: yuv.YuvBatch([yuv.YuvFrame(y[b], c[b]) for b in range(len(y))], "NV12", matrix)      # noqa: E731
    engine.upload_yuv(as_batch(Y, UV))
    assert np.array_equal(engine.get_frames(), want)
    rng = np.random.default_rng(4)
    ye, ce = rng.integers(0, 256, (4, 1024, 2), dtype=np.uint8), rng.integers(0, 256, (4, 512, 2), dtype=np.uint8)
    planes = (np.concatenate([Y, ye], axis=2), np.concatenate([UV, ce], axis=2), None)
    engine.upload_yuv(as_batch(planes[0], planes[1]))
    got = engine.get_frames()
    assert got.shape == (4, 1024, 4098, 3)
    assert np.array_equal(got[:, :, :4096], want) and np.array_equal(got[:, :, 4096:], yuv_model.frames((ye, ce, None), "NV12", matrix))


@pytest.mark.parametrize("layout", ["NV12", "I420"])
def test_device_surfaces_of_a_decoder_pool(fresh_engine, layout):
    """pitch 256, 8 padding rows between the Y and the chroma planes, frames in reverse address order; blocking and staged"""
    eng = fresh_engine
    planes = _planes(np.random.default_rng(12), 3, 36, 80, layout)
    want = yuv_model.frames(planes, layout, "BT709")
    dev, keep = _device_batch(planes, layout, "BT709", y_pitch=256, c_pitch=256, gap_rows=8, reverse=True)
    assert dev[0].y > dev[1].y > dev[2].y
    eng.upload_yuv(dev)
    a = eng.get_frames()
    eng.upload_yuv_async(dev)
    eng.swap_frames()
    b = eng.get_frames()
    eng.upload_yuv(_host_batch(planes, layout, "BT709", y_pitch=256, c_pitch=256, gap_rows=8)[0])
    c = eng.get_frames()
    assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want)
    del keep


def test_staging_discipline(fresh_engine):
    eng = fresh_engine
    rng = np.random.default_rng(21)
    old = rng.integers(0, 256, (2, 12, 20, 3), dtype=np.uint8)
    p1, p2 = _planes(rng, 3, 6, 10, "NV12"), _planes(rng, 2, 4, 32, "I420")
    b1, b2 = _host_batch(p1, "NV12", "BT601")[0], _host_batch(p2, "I420", "JFIF")[0]
    eng.upload_frames(old)
    eng.upload_yuv_async(b1)
    assert any(f.y is k.y for f in b1 for keep in eng._yuv_keep for k in keep)      # the staged planes are held while the copy may run
    assert np.array_equal(eng.get_frames(), old)                 # before the swap: still the old batch, read while the new one was staged
    eng.swap_frames()
    assert np.array_equal(eng.get_frames(), yuv_model.frames(p1, "NV12", "BT601"))
    # two staged uploads in a row: the second one stays
    eng.upload_yuv_async(b1)
    eng.upload_yuv_async(b2)
    eng.swap_frames()
    assert np.array_equal(eng.get_frames(), yuv_model.frames(p2, "I420", "JFIF"))
    # a refused call leaves the staged batch staged
    eng.upload_yuv_async(b1)
    bad = _host_batch(p2, "I420", "JFIF")[0]
    bad.matrix = "BT2020"
    with pytest.raises(ValueError):
        eng.upload_yuv_async(bad)                                # (refused by YuvBatch: never reaches the library)
    d = native.FrpYuvDesc(C.sizeof(native.FrpYuvDesc), 0, 7, 0, 10, 6, 10, 10)
    y = np.zeros(200, np.uint8)
    ptrs = (C.c_void_p * 3)(y.ctypes.data, y.ctypes.data, None)
    assert eng._lib.frp_upload_yuv_async(eng._h, C.byref(d), ptrs, 1) == -1
    assert b"matrix" in eng._lib.frp_last_error(eng._h)
    eng.swap_frames()
    assert np.array_equal(eng.get_frames(), yuv_model.frames(p1, "NV12", "BT601"))
    with pytest.raises(native.FrpError, match="no staged frames"):
        eng.swap_frames()


@pytest.mark.parametrize("staged", [False, True])
def test_neighbours_untouched(fresh_engine, staged):
    eng = fresh_engine
    big = np.full((4, 40, 64, 3), 0xA5, np.uint8)
    eng.upload_frames(big)
    if staged:                                                    # both frame buffers of the handle: 0xA5 at the larger size
        eng.upload_frames_async(big)
        eng.swap_frames()
    planes = _planes(np.random.default_rng(31), 2, 6, 10, "NV12")
    batch = _host_batch(planes, "NV12", "BT601")[0]
    if staged:
        eng.upload_yuv_async(batch)
        eng.swap_frames()
    else:
        eng.upload_yuv(batch)
    assert np.array_equal(eng.get_frames(0, 2), yuv_model.frames(planes, "NV12", "BT601"))
    with pytest.raises(native.FrpError, match="outside"):
        eng.get_frames(0, 3)                                      # the batch is B frames, whatever the buffer held before
    bgr = np.random.default_rng(32).integers(0, 256, (3, 40, 64, 3), dtype=np.uint8)
    eng.upload_frames(bgr)
    assert np.array_equal(eng.get_frames(), bgr)
    assert np.array_equal(eng.get_frames(1, 2), bgr[1:])


def _desc(**kw):
    f = dict(struct_size=C.sizeof(native.FrpYuvDesc), layout=0, matrix=0, flags=0, width=10, height=6, y_pitch=10, c_pitch=10)
    f.update(kw)
    return native.FrpYuvDesc(*[f[n] for n, _ in native.FrpYuvDesc._fields_])


REFUSALS = {
    "struct_size": (_desc(struct_size=36), 1, None, "struct_size"),
    "layout": (_desc(layout=4), 1, None, "layout"),
    "layout_negative": (_desc(layout=-1), 1, None, "layout"),
    "matrix": (_desc(matrix=3), 1, None, "matrix"),
    "flags": (_desc(flags=2), 1, None, "flags"),
    "width_odd": (_desc(width=9), 1, None, "width"),
    "width_zero": (_desc(width=0), 1, None, "width"),
    "height_odd": (_desc(height=5), 1, None, "height"),
    "height_negative": (_desc(height=-2), 1, None, "height"),
    "y_pitch": (_desc(y_pitch=9), 1, None, "y_pitch"),
    "c_pitch_semi_planar": (_desc(c_pitch=9), 1, None, "c_pitch"),
    "c_pitch_planar": (_desc(layout=2, c_pitch=4), 1, None, "c_pitch"),
    "plane_y_null": (_desc(), 2, (1, 0), "planes[1][0]"),
    "plane_uv_null": (_desc(), 2, (0, 1), "planes[0][1]"),
    "plane_v_null": (_desc(layout=3), 2, (1, 2), "planes[1][2]"),
    "B_zero": (_desc(), 0, None, "B must"),
    "B_too_large": (_desc(), 1025, None, "B must"),
}


@pytest.mark.parametrize("rule", list(REFUSALS))
def test_refusals_name_the_field(engine, rule):
    d, B, null_at, field = REFUSALS[rule]
    mem = np.zeros(256, np.uint8)
    semi = d.layout in (0, 1)
    n = max(B, 1)
    ptrs = (C.c_void_p * (3 * n))(*([mem.ctypes.data, mem.ctypes.data, None if semi else mem.ctypes.data] * n))
    if null_at is not None:
        ptrs[3 * null_at[0] + null_at[1]] = None
    for fn in (engine._lib.frp_upload_yuv, engine._lib.frp_upload_yuv_async):
        assert fn(engine._h, C.byref(d), ptrs, B) == -1, rule
        assert field in engine._lib.frp_last_error(engine._h).decode(), rule


def test_refusals_null_arguments_and_get_frames(fresh_engine):
    eng = fresh_engine
    lib, d = eng._lib, _desc()
    mem = np.zeros(256, np.uint8)
    ptrs = (C.c_void_p * 3)(mem.ctypes.data, mem.ctypes.data, None)
    out = np.zeros(4 * 6 * 10 * 3, np.uint8)
    assert lib.frp_get_frames(eng._h, out.ctypes.data, out.nbytes, 0, 1) == -1 and b"resident" in lib.frp_last_error(eng._h)
    for fn in (lib.frp_upload_yuv, lib.frp_upload_yuv_async):
        assert fn(eng._h, None, ptrs, 1) == -1 and b"desc" in lib.frp_last_error(eng._h)
        assert fn(eng._h, C.byref(d), None, 1) == -1 and b"planes" in lib.frp_last_error(eng._h)
    with pytest.raises(native.FrpError, match="no staged frames"):
        eng.swap_frames()                                         # nothing was queued by any of them
    eng.upload_yuv(_host_batch(_planes(np.random.default_rng(1), 2, 6, 10, "NV12"), "NV12", "BT601")[0])
    for first, n in ((0, 3), (2, 1), (-1, 1), (1, 0), (1, 2)):
        assert lib.frp_get_frames(eng._h, out.ctypes.data, out.nbytes, first, n) == -1 and b"outside" in lib.frp_last_error(eng._h), (first, n)
    assert lib.frp_get_frames(eng._h, out.ctypes.data, 2 * 180 - 1, 0, 2) == -1 and b"out_bytes" in lib.frp_last_error(eng._h)
    assert lib.frp_get_frames(eng._h, out.ctypes.data, 2 * 180, 0, 2) == 0


def test_one_real_size(engine):
    planes = _planes(np.random.default_rng(41), 2, 1080, 1920, "NV12")
    want = yuv_model.frames(planes, "NV12", "BT709")
    batch = _host_batch(planes, "NV12", "BT709", y_pitch=2048, c_pitch=2048)[0]
    engine.upload_yuv(batch)
    a = engine.get_frames()
    engine.upload_yuv(batch)
    b = engine.get_frames()
    assert np.array_equal(a, want) and np.array_equal(a, b)


def _rgb_to_nv12(rgb):
    """a still -> full-range (JFIF) Y and interleaved UV planes, chroma averaged over 2 x 2: only a plausible picture is needed"""
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    sub = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean((1, 3))      # noqa: E731
    u, v = 128 + 0.564 * sub(b - y), 128 + 0.713 * sub(r - y)
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)                            # noqa: E731
    return q(y), np.stack([q(u), q(v)], -1).reshape(u.shape[0], -1)


def test_through_the_service(engine):
    from PIL import Image
    raw, blob = get_raw_and_blob((1, 1, 1, 1), (1, 1, 1, 1))
    engine.load_weights(blob)
    with open(os.path.join(HERE, "golden", "stills", "c420_q85.jpg"), "rb") as f:
        rgb = np.asarray(Image.open(io.BytesIO(f.read())).convert("RGB"))
    assert rgb.shape == (96, 128, 3)
    pics = [rgb, rgb[:, ::-1], rgb[::-1]]
    Y, UV = (np.stack(a) for a in zip(*[_rgb_to_nv12(p) for p in pics]))
    batch = yuv.YuvBatch([yuv.YuvFrame(Y[i], UV[i]) for i in range(3)], "NV12", "JFIF")
    pixels = yuv_model.frames((Y, UV, None), "NV12", "JFIF")
    assert np.abs(pixels[0, ..., ::-1].astype(int) - rgb).mean() < 6          # the helper made the picture, not noise
    fs = FaceService(engine=engine)
    fs.ENCODINGS.clear()
    try:
        rng = np.random.default_rng(0)
        for i in range(6):
            fs.store_face(f"p{i}", rng.standard_normal(512))
        for quality in (False, True):
            got = fs.process_frames(batch, max_faces=4, det_thresh=0.02, quality=quality)
            want = fs.process_frames(pixels, max_faces=4, det_thresh=0.02, quality=quality)
            assert len(got) == len(want) == 3 and sum(len(f) for f in want) > 0
            for fa, fb in zip(got, want):
                assert len(fa) == len(fb)
                for x, y in zip(fa, fb):
                    assert x.keys() == y.keys()
                    for k in x:
                        assert np.array_equal(x[k], y[k]) if isinstance(x[k], np.ndarray) else x[k] == y[k], k
        fs.process_frames(batch, max_faces=4, det_thresh=0.02)
        assert np.array_equal(engine.get_frames(), pixels)                      # what the YUV route left resident: the model's pixels
        got = list(fs.process_stream(iter([batch, batch]), max_faces=4, det_thresh=0.02))
        assert len(got) == 2 and [len(f) for f in got[0]] == [len(f) for f in want]
    finally:
        fs.ENCODINGS.clear()
