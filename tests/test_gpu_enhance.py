"""GPU tests of the snapshot enhancer (csrc/enhance_kernels.hip, frp_enhance_pixels / frp_encode_jpeg_enhanced, Engine.enhance_pixels /
encode_jpeg_enhanced) and of the service methods on top of it.  Integer arithmetic throughout: every comparison is exact - pixels
byte for byte against the numpy model (tests/enhance_model.py) and against Pillow on the numpy crop, files byte for byte against
Pillow's save of Pillow's enhanced image."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import enhance_model as M
import jpeg_encode_model as JM
from conftest import get_raw_and_blob
from enhance_cases import DEFAULT, PARAMS, SIZES, content
from frp_amd import face_service, native
from frp_amd.face_service import FaceService
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

SMALL = (3, 131, 97)          # B, H, W: 3 resident frames of 97 x 131
LARGE = (2, 300, 200)         # ... and a second upload of 2 frames of 200 x 300 for the cases that do not fit
RING = 5


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _plant(frames, b, top, left, img):
    """`img` into frame b at (top, left); the RING pixels around it become the complement of the crop's nearest edge pixel, so
    whatever reads a neighbour of the crop instead of clamping at its edge is far off"""
    h, w = img.shape[:2]
    H, W = frames.shape[1:3]
    ring = 255 - np.pad(img, ((RING, RING), (RING, RING), (0, 0)), mode="edge")
    t0, l0, t1, l1 = max(top - RING, 0), max(left - RING, 0), min(top + h + RING, H), min(left + w + RING, W)
    frames[b, t0:t1, l0:l1] = ring[t0 - (top - RING):t1 - (top - RING), l0 - (left - RING):l1 - (left - RING)]
    frames[b, top:top + h, left:left + w] = img
    return (b, top, left + w, top + h, left)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (what, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def _crop(frames, rect):
    b, top, right, bottom, left = rect
    return np.ascontiguousarray(frames[b, top:bottom, left:right])


def _kw(params):
    radius, percent, threshold, sharpen = params
    return dict(radius=radius, percent=percent, threshold=threshold, sharpen=sharpen)


@pytest.mark.parametrize("kind", ["noise", "ramp"])
@pytest.mark.parametrize("name", sorted(SIZES))
def test_crops_equal_the_model_and_pillow(engine, name, kind):
    """every size case as a crop at two frame corners (the first and the very last pixel of the resident buffer) and in the interior,
    for every parameter set"""
    w, h, ow, oh = SIZES[name]
    B, H, W = SMALL if (w <= SMALL[2] - 2 * RING and h <= SMALL[1] - 2 * RING) else LARGE
    frames = _noise(11, (B, H, W, 3))
    img = content(kind, h, w, seed=3)
    rects = [_plant(frames, 0, 0, 0, img), _plant(frames, B - 1, H - h, W - w, img), _plant(frames, 1, (H - h) // 2 + 1, (W - w) // 2 + 1, img)]
    for r in rects:
        assert np.array_equal(_crop(frames, r), img)
    engine.upload_frames(frames)
    for params in PARAMS:
        want = M.enhance(img, ow, oh, *params)
        _same(want, M.pillow_enhance(img, ow, oh, *params), ("model / Pillow", name, params))
        got = engine.enhance_pixels(rects, [(ow, oh)] * 3, **_kw(params))
        for where, g in zip(("first corner", "last corner", "interior"), got):
            _same(g, want, (name, kind, params, where))


@pytest.mark.parametrize("size", [(194, 262), (131, 177), (97, 131), (97, 140)])
def test_whole_frames(engine, size):
    """the crop is the frame: x2, a non-integer ratio, nothing but the mask, one axis; more than one tile per axis"""
    B, H, W = SMALL
    frames = np.stack([content("ramp", H, W, seed=5), content("noise", H, W, seed=6), content("ramp", H, W, seed=7)])
    engine.upload_frames(frames)
    got = engine.enhance_pixels([(b, 0, W, H, 0) for b in range(B)], [size] * B)
    for b in range(B):
        want = M.enhance(frames[b], *size)
        _same(want, M.pillow_enhance(frames[b], *size), ("model / Pillow", size, b))
        _same(got[b], want, (size, b))


def _raw_pixels(eng, rects, sizes, n, prm, flags, out, cap, offsets):
    r = np.ascontiguousarray(rects, np.int32)
    s = np.ascontiguousarray(sizes, np.int32)
    p = native.FrpEnhanceParams(*prm)
    return eng._lib.frp_enhance_pixels(eng._h, r.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), n, C.byref(p), flags,
                                       out.ctypes.data_as(C.c_void_p), cap, offsets.ctypes.data_as(C.c_void_p))


def _raw_jpeg(eng, rects, sizes, n, prm, q, ss, r, flags, out, cap, offsets):
    rr = np.ascontiguousarray(rects, np.int32)
    s = np.ascontiguousarray(sizes, np.int32)
    p = native.FrpEnhanceParams(*prm)
    return eng._lib.frp_encode_jpeg_enhanced(eng._h, rr.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), n, C.byref(p), q, ss, r, flags,
                                             out.ctypes.data_as(C.c_void_p), cap, offsets.ctypes.data_as(C.c_void_p))


SEVEN = [((0, 3, 60, 40, 7), (106, 74)), ((2, 100, 97, 131, 80), (17, 31)), ((1, 0, 97, 131, 0), (150, 140)), ((0, 50, 30, 51, 29), (2, 2)),
         ((2, 10, 90, 75, 20), (70, 130)), ((1, 64, 33, 129, 1), (65, 65)), ((0, 5, 97, 40, 0), (200, 35))]
PRM = (1.0, 120, 3, 1)


def test_seven_rectangles_in_one_call_and_the_bytes_behind_them(engine):
    B, H, W = SMALL
    frames = _noise(21, (B, H, W, 3))
    frames[1] = content("ramp", H, W, seed=8)
    engine.upload_frames(frames)
    rects, sizes = [r for r, _ in SEVEN], [s for _, s in SEVEN]
    together = engine.enhance_pixels(rects, sizes)
    for i, (r, s) in enumerate(SEVEN):
        single = engine.enhance_pixels([r], [s])[0]
        _same(together[i], single, ("one call / single calls", i))
        _same(together[i], M.pillow_enhance(_crop(frames, r), *s), ("Pillow", i))
    again = engine.enhance_pixels(rects, sizes)
    assert all(np.array_equal(a, b) for a, b in zip(together, again))
    # the raw entry: offsets, the images back to back, nothing behind offsets[n]
    total = sum(3 * s[0] * s[1] for s in sizes)
    out = np.full(total + 4099, 0xA5, np.uint8)
    offsets = np.full(8, -7, np.int64)
    assert _raw_pixels(engine, rects, sizes, 7, PRM, 0, out, out.size, offsets) == 0
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([3 * s[0] * s[1] for s in sizes])]).tolist()
    assert out[:total].tobytes() == b"".join(t.tobytes() for t in together)
    assert (out[total:] == 0xA5).all()
    # exactly enough goes through, one byte less is refused with the sizes reported and nothing written
    out[:] = 0xA5
    offsets[:] = -7
    assert _raw_pixels(engine, rects, sizes, 7, PRM, 0, out, total - 1, offsets) == -1
    assert offsets[7] == total and offsets[0] == 0 and (out == 0xA5).all()
    assert _raw_pixels(engine, rects, sizes, 7, PRM, 0, out, total, offsets) == 0
    assert out[:total].tobytes() == b"".join(t.tobytes() for t in together) and (out[total:] == 0xA5).all()


def _pil_file(rgb, quality, ss="4:2:0", **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=JM.PIL_SUBSAMPLING[ss], **kw)
    return buf.getvalue()


def test_enhanced_jpeg_files_equal_pillows(engine):
    B, H, W = SMALL
    frames = np.stack([content("ramp", H, W, seed=31), content("noise", H, W, seed=32), content("ramp", H, W, seed=33)])
    engine.upload_frames(frames)
    jobs = [((0, 0, W, H, 0), (194, 262)), ((1, 20, 80, 70, 10), (99, 71)), ((2, 1, 34, 6, 31), (7, 9)), ((2, 40, 81, 73, 40), (41, 33))]
    rects, sizes = [r for r, _ in jobs], [s for _, s in jobs]
    for ss in ("4:2:0", "4:4:4"):
        got = engine.encode_jpeg_enhanced(rects, sizes, quality=85, subsampling=ss)
        assert len(got) == len(jobs)
        for i, (r, s) in enumerate(jobs):
            enhanced_rgb = M.pillow_enhance(np.ascontiguousarray(_crop(frames, r)[..., ::-1]), *s)      # resident frames are BGR
            assert got[i] == _pil_file(enhanced_rgb, 85, ss), (ss, i)
            if ss == "4:2:0":
                # what the reference itself saves (optimize=True) has other Huffman tables and the same quantised coefficients
                ref = _pil_file(enhanced_rgb, 85, ss, optimize=True)
                assert ref != got[i]
                assert np.array_equal(native.jpeg_coefficients(got[i])[1], native.jpeg_coefficients(ref)[1]), i
    as_rgb = engine.encode_jpeg_enhanced(rects, sizes, quality=85, rgb=True)
    for i, (r, s) in enumerate(jobs):
        assert as_rgb[i] == _pil_file(M.pillow_enhance(_crop(frames, r), *s), 85), i
    # the file and the pixel entry agree, and the plain encoder's files are what they were
    px = engine.enhance_pixels(rects[:1], sizes[:1])[0]
    assert engine.encode_jpeg_enhanced(rects[:1], sizes[:1], quality=85)[0] == _pil_file(np.ascontiguousarray(px[..., ::-1]), 85)
    assert engine.encode_jpeg(rects, quality=85) == [JM.pil_encode(np.ascontiguousarray(_crop(frames, r)[..., ::-1]), 85) for r in rects]
    # resample only, restart markers, and a first guess that is too small (noise at quality 100)
    noisy = engine.encode_jpeg_enhanced([(1, 0, W, H, 0)] * 2, [(W, H)] * 2, sharpen=False, quality=100, subsampling="4:4:4")
    assert noisy[0] == noisy[1] == JM.pil_encode(np.ascontiguousarray(frames[1, :, :, ::-1]), 100, "4:4:4")
    assert engine.encode_jpeg_enhanced(rects[1:2], sizes[1:2], quality=85, restart_mcus=3)[0] == \
        JM.pil_encode(M.pillow_enhance(np.ascontiguousarray(_crop(frames, rects[1])[..., ::-1]), *sizes[1]), 85, "4:2:0", 3)


def test_refusals_write_nothing_and_name_the_rectangle(engine, fresh_engine):
    frames = _noise(9, (2, 33, 50, 3))
    B, H, W, _ = frames.shape
    engine.upload_frames(frames)
    good, gsize = (1, 2, 40, 30, 4), (72, 56)
    total = 3 * gsize[0] * gsize[1]
    out = np.full(2 * total + 4096, 0xA5, np.uint8)
    offsets = np.full(3, -7, np.int64)
    err = lambda eng: eng._lib.frp_last_error(eng._h)

    def refused(what, rects, sizes, n=2, prm=PRM, flags=0, q=85, ss=420, r=0, eng=engine):
        for rc in (_raw_pixels(eng, rects, sizes, n, prm, flags, out, out.size, offsets),
                   _raw_jpeg(eng, rects, sizes, n, prm, q, ss, r, flags, out, out.size, offsets)):
            assert rc == -1, what
            assert (out == 0xA5).all() and (offsets == -7).all(), what

    for rect in [(-1, 2, 40, 30, 4), (B, 2, 40, 30, 4), (1, -1, 40, 30, 4), (1, 30, 40, 30, 4), (1, 2, 40, H + 1, 4), (1, 2, 40, 30, -1),
                 (1, 2, 40, 30, 40), (1, 2, W + 1, 30, 4)]:
        refused(rect, [good, rect], [gsize, gsize])
        assert b"rectangle 1 " in err(engine), rect
        with pytest.raises(FrpError):
            engine.enhance_pixels([rect], [gsize])
    for size in [(35, 56), (72, 27), (65536, 56), (72, 65536), (0, 0), (-1, 56), (4097, 4096), (65535, 65535)]:     # good is 36 x 28
        refused(size, [good, good], [gsize, size])
        assert b"rectangle 1 " in err(engine), size
        with pytest.raises(FrpError):
            engine.encode_jpeg_enhanced([good], [size])
    assert native.ENHANCE_MAX_PIXELS == 1 << 24 and 4097 * 4096 > native.ENHANCE_MAX_PIXELS
    for prm in [(-0.5, 120, 3, 1), (float("nan"), 120, 3, 1), (native.ENHANCE_MAX_RADIUS + 0.01, 120, 3, 1), (float("inf"), 120, 3, 1),
                (1.0, -1, 3, 1), (1.0, 120, -1, 1), (-1.0, 120, 3, 0)]:
        refused(prm, [good], [gsize], n=1, prm=prm)
    for flags in (native.FLAG_FORCED_K, native.FLAG_RGB | native.FLAG_NO_MATCH, 1 << 31):
        refused(flags, [good], [gsize], n=1, flags=flags)
    refused("n < 0", [good], [gsize], n=-1)
    refused("no resident frames", [good], [gsize], n=1, eng=fresh_engine)
    assert b"no resident frames" in err(fresh_engine)
    # the encoder's own arguments, before anything is launched
    for q, ss, r in [(0, 420, 0), (101, 420, 0), (85, 422, 0), (85, 420, -1), (85, 420, 65536)]:
        assert _raw_jpeg(engine, [good], [gsize], 1, PRM, q, ss, r, 0, out, out.size, offsets) == -1, (q, ss, r)
        assert (out == 0xA5).all() and (offsets == -7).all()
    # n == 0
    assert _raw_pixels(engine, [good], [gsize], 0, PRM, 0, out, out.size, offsets) == 0 and offsets[0] == 0 and (out == 0xA5).all()
    offsets[:] = -7
    assert _raw_jpeg(engine, [good], [gsize], 0, PRM, 85, 420, 0, 0, out, out.size, offsets) == 0 and offsets[0] == 0 and (out == 0xA5).all()
    assert engine.enhance_pixels(np.zeros((0, 5), np.int32), np.zeros((0, 2), np.int32)) == []
    assert engine.encode_jpeg_enhanced(np.zeros((0, 5), np.int32), np.zeros((0, 2), np.int32)) == []
    # files too small by one byte: refused, sizes reported, nothing written; exactly enough goes through
    size = len(engine.encode_jpeg_enhanced([good], [gsize])[0])
    offsets[:] = -7
    assert _raw_jpeg(engine, [good, good], [gsize, gsize], 2, PRM, 85, 420, 0, 0, out, 2 * size - 1, offsets) == -1
    assert offsets.tolist() == [0, size, 2 * size] and (out == 0xA5).all()
    assert _raw_jpeg(engine, [good, good], [gsize, gsize], 2, PRM, 85, 420, 0, 0, out, 2 * size, offsets) == 0
    ref = _pil_file(M.pillow_enhance(np.ascontiguousarray(_crop(frames, good)[..., ::-1]), *gsize), 85)
    assert out[:2 * size].tobytes() == ref + ref and (out[2 * size:] == 0xA5).all()
    # the radius cap itself is accepted
    got = engine.enhance_pixels([good], [gsize], radius=native.ENHANCE_MAX_RADIUS, percent=150, threshold=3)[0]
    _same(got, M.pillow_enhance(_crop(frames, good), *gsize, native.ENHANCE_MAX_RADIUS, 150, 3), "radius cap")


def _scene(rng, B, H, W):
    base = rng.integers(0, 255, size=(B, H // 16, W // 16, 3)).astype(np.float32)
    base = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    return np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)


def test_results_of_the_last_pass_stay_fetchable(fresh_engine):
    engine = fresh_engine
    rng = np.random.default_rng(12)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 6
    frames = _scene(rng, B, H, W)
    engine.gallery_set(rng.standard_normal((300, 512)).astype(np.float32))
    engine.upload_frames(frames)
    engine.process_resident(K, flags=native.FLAG_FORCED_K)
    rects, sizes = [(1, 17, 200, 99, 31), (0, 0, W, H, 0)], [(338, 164), (300, 225)]
    want = [M.pillow_enhance(_crop(frames, r), *s) for r, s in zip(rects, sizes)]
    queued = engine.enhance_pixels(rects, sizes)                     # queued behind the pending pass, before anything was fetched
    for g, w_ in zip(queued, want):
        _same(g, w_, "queued")
    files = engine.encode_jpeg_enhanced(rects, sizes)
    assert files == [_pil_file(np.ascontiguousarray(w_[..., ::-1]), 85) for w_ in want]
    before = engine.fetch_results()
    assert before["counts"].tolist() == [K] * B
    with pytest.raises(FrpError):
        engine.enhance_pixels(rects, [(10, 10)] * 2)                 # a refusal in between changes nothing either
    assert engine.encode_jpeg_enhanced(rects, sizes) == files
    after = engine.fetch_results()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


def test_service_snapshot_thumbnails_and_enhance_snapshot(engine, monkeypatch):
    for k in ("ENHANCER_UPSCALE_FACTOR", "ENHANCER_MAX_PIXELS", "ENHANCER_JPEG_QUALITY", "ENHANCER_SHARPEN"):
        monkeypatch.delenv(k, raising=False)
    frames = np.stack([content("ramp", 64, 96, seed=41), content("noise", 64, 96, seed=42)])
    engine.upload_frames(frames)
    fs = FaceService(engine=engine)

    def pillow(bgr, quality, upscale=2.0, max_pixels=4_000_000, sharpen=True):
        h, w = bgr.shape[:2]
        nw, nh = M.enhanced_size(w, h, upscale, max_pixels)
        size = (nw, nh) if nw > w or nh > h else (w, h)
        return _pil_file(M.pillow_enhance(np.ascontiguousarray(bgr[..., ::-1]), *size, sharpen=sharpen), quality)

    # the reference's defaults: x2, UnsharpMask(1, 120, 3), quality 85
    snap = fs.enhance_snapshot(1)
    assert snap == pillow(frames[1], 85) and Image.open(io.BytesIO(snap)).size == (192, 128)
    assert fs.snapshot_jpeg(0, quality=70, enhance=True) == pillow(frames[0], 70)
    assert fs.snapshot_jpeg(0, quality=70) == JM.pil_encode(np.ascontiguousarray(frames[0, :, :, ::-1]), 70)      # enhance=False: as before
    faces = [(0, (10, 50, 40, 20)), (1, (-5, 110, 30, 80)), (1, (50, 20, 70, 0))]
    thumbs = fs.face_thumbnails(faces, margin=0.5, quality=90, enhance=True)
    assert [Image.open(io.BytesIO(t)).size for t in thumbs] == [(120, 110), (62, 96), (60, 48)]
    assert thumbs[0] == pillow(frames[0, 0:55, 5:65], 90)
    assert thumbs[1] == pillow(frames[1, 0:48, 65:96], 90)
    plain = fs.face_thumbnails(faces, margin=0.5, quality=90)
    assert plain[0] == JM.pil_encode(np.ascontiguousarray(frames[0, 0:55, 5:65, ::-1]), 90)
    # the pixel cap (96 x 64 -> 120 x 80), another factor, quality and no mask
    monkeypatch.setenv("ENHANCER_MAX_PIXELS", "9600")
    monkeypatch.setenv("ENHANCER_JPEG_QUALITY", "60")
    assert face_service.enhanced_size(96, 64, 2.0, 9600) == (120, 80)
    snap = fs.enhance_snapshot(0)
    assert snap == pillow(frames[0], 60, max_pixels=9600) and Image.open(io.BytesIO(snap)).size == (120, 80)
    monkeypatch.setenv("ENHANCER_SHARPEN", "no")
    monkeypatch.setenv("ENHANCER_UPSCALE_FACTOR", "1.25")
    monkeypatch.setenv("ENHANCER_MAX_PIXELS", "4000000")
    assert fs.enhance_snapshot(1) == pillow(frames[1], 60, upscale=1.25, sharpen=False)
    # a cap below the frame: nothing is resampled, the mask still runs (enhancer.py:80-85)
    monkeypatch.setenv("ENHANCER_SHARPEN", "true")
    monkeypatch.setenv("ENHANCER_MAX_PIXELS", "1000")
    snap = fs.enhance_snapshot(1)
    assert snap == pillow(frames[1], 60, upscale=1.25, max_pixels=1000) and Image.open(io.BytesIO(snap)).size == (96, 64)
    # failures are logged, not raised
    monkeypatch.setenv("ENHANCER_JPEG_QUALITY", "not a number")
    assert fs.enhance_snapshot(0) is None
    monkeypatch.setenv("ENHANCER_JPEG_QUALITY", "85")
    assert fs.snapshot_jpeg(9, enhance=True) is None and fs.face_thumbnails([(5, (0, 10, 10, 0))], enhance=True) == []


def test_a_1080p_frame_at_the_reference_defaults(engine):
    """1920 x 1080 -> 2667 x 1500 (enhanced_size at the defaults) against Pillow directly: 42 x 47 tiles, offsets past 2^23"""
    rng = np.random.default_rng(1080)
    frame = np.ascontiguousarray(_scene(rng, 1, 1088, 1920)[:, :1080])
    engine.upload_frames(frame)
    size = M.enhanced_size(1920, 1080)
    assert size == (2667, 1500)
    want = M.pillow_enhance(frame[0], *size)
    got = engine.enhance_pixels([(0, 0, 1920, 1080, 0)], [size])[0]
    _same(got, want, "1080p")
    assert engine.encode_jpeg_enhanced([(0, 0, 1920, 1080, 0)], [size])[0] == _pil_file(np.ascontiguousarray(want[..., ::-1]), 85)
