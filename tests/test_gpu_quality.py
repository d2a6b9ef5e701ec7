"""GPU tests of the face-quality kernel (csrc/quality_kernels.hip, frp_face_quality, Engine.face_quality) and of the service keywords on
top of it.  The four sums per rectangle are integers over u8 data: every comparison is `==` on int64 against the numpy model
(tests/quality_model.py), whatever the summation order."""
import ctypes as C

import numpy as np
import pytest

import quality_model
from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.face_service import FaceService, box_to_location
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

TH, TW = native.QUALITY_TILE_H, native.QUALITY_TILE_W


def _noise(seed, shape):
    a = np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


# 3x97x131: an odd width - rows start at every dword phase - and 3*97*131*3 = 114363 = 3 mod 4: the buffer ends in a partial dword
FRAMES = {"odd": _noise(1, (3, 97, 131, 3)), "even": _noise(2, (2, 64, 256, 3)),
          "two_tiles_and_a_bit": _noise(3, (1, 2 * TH + 8, 2 * TW + 8, 3))}


def _rects(name):
    B, H, W, _ = FRAMES[name].shape
    r = []
    for f in (0, B - 1):                                                    # 1x1 at each corner of the first and the last frame
        r += [(f, 0, 1, 1, 0), (f, 0, W, 1, W - 1), (f, H - 1, 1, H, 0), (f, H - 1, W, H, W - 1)]
    r += [(0, 5, 29, 6, 20), (B - 1, 5, 21, 14, 20), (B - 1, 50, 52, 52, 50)]      # 1x9, 9x1, 2x2
    r += [(B - 1, 10, left + 37, 30, left) for left in (0, 1, 2, 3)]        # every byte phase of the crop's first column
    r += [(B - 1, H - 30, W, H, W - 41)]                                    # ends at the last pixel of the last frame
    r += [(f, 0, W, H, 0) for f in range(B)]                                # whole frames
    if H >= TH + 3 and W >= TW + 5:
        r += [(0, 3, 5 + TW, 3 + TH, 5)]                                    # exactly one tile
    if H >= TH + 1:
        r += [(0, H - TH - 1, 43, H, 6)]                                    # TH + 1 rows
    if W >= TW + 8:
        r += [(B - 1, 1, 7 + TW + 1, 20, 7)]                                # TW + 1 columns
    if H >= 2 * TH + 3 and W >= 2 * TW + 5:
        r += [(0, 2, 3 + 2 * TW + 5, 2 + 2 * TH + 3, 3)]                    # (2 TH + 3) x (2 TW + 5): a 3 x 3 grid of tiles
    r += [(0, 10, 60, 50, 20), (0, 30, 100, 62, 40)]                        # two overlapping rectangles
    r += [(B - 1, 5, 50, 40, 10)] * 2                                       # the same rectangle twice
    return np.array(r, np.int32)


@pytest.mark.parametrize("name", list(FRAMES))
def test_sums_equal_the_integer_model(engine, name):
    frames = FRAMES[name]
    engine.upload_frames(frames)
    rects = _rects(name)
    if name == "two_tiles_and_a_bit":
        assert (rects[:, 3] - rects[:, 1] == 2 * TH + 3).any()
    for rgb in (False, True):
        got = engine.face_quality(rects, rgb=rgb)
        want = quality_model.sums_of(frames, rects, rgb)
        assert got.dtype == np.int64 and got.shape == want.shape
        bad = np.argwhere((got != want).any(axis=1))
        assert len(bad) == 0, (rgb, rects[bad[0, 0]].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    assert engine.face_quality(np.zeros((0, 5), np.int32)).shape == (0, 4)          # n == 0: FRP_OK


def test_forty_rectangles_over_three_frames_colour_order_and_determinism(engine):
    frames = FRAMES["odd"]
    B, H, W, _ = frames.shape
    rng = np.random.default_rng(40)
    rects = []
    for i in range(40):
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        rects.append((i % B, top, left + w, top + h, left))
    engine.upload_frames(frames)
    bgr, rgb = engine.face_quality(rects, rgb=False), engine.face_quality(rects, rgb=True)
    assert np.array_equal(bgr, quality_model.sums_of(frames, rects, False))
    assert np.array_equal(rgb, quality_model.sums_of(frames, rects, True))
    assert (bgr != rgb).any(axis=1).all()                       # the same bytes in the other channel order: other sums, everywhere
    assert np.array_equal(engine.face_quality(rects, rgb=False), bgr)          # a second call: the same


def test_sums_beyond_32_bits(engine):
    """a 0/255 checkerboard: |lap| = 1020 at every interior pixel, L2 = 6.8e10 for 256 x 256 and 2.2e12 for 1080 x 1920"""
    yy, xx = np.mgrid[0:1080, 0:1920]
    frames = np.ascontiguousarray(np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], (1, 1080, 1920, 3)))
    rects = [(0, 300, 777 + 256, 300 + 256, 777), (0, 0, 1920, 1080, 0)]
    want = quality_model.sums_of(frames, rects)
    assert want[0, 3] > 6e10 and want[1, 3] > 2e12
    engine.upload_frames(frames)
    assert np.array_equal(engine.face_quality(rects), want)


@pytest.mark.parametrize("where,expect", [
    ("corner", (255, 255 * 255, -510, 1020 * 1020 + 2 * 255 * 255)),                  # (0, 0): two neighbours inside the crop
    ("next_to_corner", (255, 255 * 255, 510, 1020 * 1020 + 2 * 510 * 510 + 2 * 255 * 255)),   # (1, 1): rows / columns 0 see it twice
    ("tile_seam", (255, 255 * 255, 0, 1020 * 1020 + 4 * 255 * 255)),
    ("interior", (255, 255 * 255, 0, 1020 * 1020 + 4 * 255 * 255))])
def test_impulse_closed_form(engine, where, expect):
    """one white pixel in a black crop; the frame around the crop is grey, so a kernel that reflected at the FRAME's edge, or
    read the crop's neighbours instead of reflecting, would see it.  Pins BORDER_REFLECT_101 and the halo across a tile seam."""
    H, W = 2 * TH + 8, 2 * TW + 8
    top, left, h, w = 3, 5, 2 * TH, 2 * TW
    y, x = {"corner": (0, 0), "next_to_corner": (1, 1), "tile_seam": (TH - 1, TW), "interior": (10, 10)}[where]
    frames = np.full((1, H, W, 3), 90, np.uint8)
    frames[0, top:top + h, left:left + w] = 0
    frames[0, top + y, left + x] = 255
    rect = [(0, top, left + w, top + h, left)]
    assert quality_model.sums_of(frames, rect)[0].tolist() == list(expect)      # the model agrees with the closed form
    engine.upload_frames(frames)
    assert engine.face_quality(rect)[0].tolist() == list(expect)


def _raw_call(eng, rects, n, flags, sums):
    r = np.ascontiguousarray(rects, np.int32)
    return eng._lib.frp_face_quality(eng._h, r.ctypes.data_as(C.c_void_p), n, flags, sums.ctypes.data_as(C.c_void_p))


def test_refusals_write_nothing(engine, fresh_engine):
    frames = FRAMES["odd"]
    B, H, W, _ = frames.shape
    engine.upload_frames(frames)
    good = (1, 10, 50, 40, 20)
    bad = [(-1, 10, 50, 40, 20), (B, 10, 50, 40, 20), (1, -1, 50, 40, 20), (1, 40, 50, 40, 20), (1, 41, 50, 40, 20), (1, 10, 50, H + 1, 20),
           (1, 10, 50, 40, -1), (1, 10, 50, 40, 50), (1, 10, 50, 40, 51), (1, 10, W + 1, 40, 20)]
    poison = np.int64(0x5A5A5A5A5A5A5A5A)
    for rect in bad:
        sums = np.full((2, 4), poison, np.int64)
        assert _raw_call(engine, [good, rect], 2, 0, sums) == -1, rect
        assert (sums == poison).all(), rect
        assert b"rectangle 1 " in engine._lib.frp_last_error(engine._h)
        with pytest.raises(FrpError):
            engine.face_quality([rect])
    sums = np.full((1, 4), poison, np.int64)
    assert _raw_call(engine, [good], -1, 0, sums) == -1
    for flags in (native.FLAG_FORCED_K, native.FLAG_NO_MATCH | native.FLAG_RGB, 1 << 31):
        assert _raw_call(engine, [good], 1, flags, sums) == -1
    assert _raw_call(fresh_engine, [good], 1, 0, sums) == -1 and b"no resident frames" in fresh_engine._lib.frp_last_error(fresh_engine._h)
    assert (sums == poison).all()
    assert _raw_call(engine, [good], 1, native.FLAG_RGB, sums) == 0                     # ... and the good one goes through
    assert np.array_equal(sums, quality_model.sums_of(frames, [good], True))


def _scene(rng, B, H, W):
    base = rng.integers(0, 255, size=(B, H // 16, W // 16, 3)).astype(np.float32)
    base = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    return np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)


def test_results_of_the_last_pass_stay_fetchable(fresh_engine):
    engine = fresh_engine
    rng = np.random.default_rng(11)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 6
    frames = _scene(rng, B, H, W)
    G = rng.standard_normal((300, 512)).astype(np.float32)
    engine.gallery_set(G)
    engine.set_within(0.1, 64)
    engine.upload_frames(frames)
    engine.process_resident(K, flags=native.FLAG_FORCED_K | native.FLAG_WITHIN)
    rects = [(b, 0, W, H, 0) for b in range(B)] + [(1, 17, 200, 99, 31)]
    queued = engine.face_quality(rects)                          # queued behind the pending pass, before anything was fetched
    assert np.array_equal(queued, quality_model.sums_of(frames, rects))
    before, within_before = engine.fetch_results(), engine.fetch_within()
    assert before["counts"].tolist() == [K] * B
    assert np.array_equal(engine.face_quality(rects), queued)
    after, within_after = engine.fetch_results(), engine.fetch_within()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    for a, b in zip(within_before, within_after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_service_quality_on_the_device(fresh_engine):
    """FaceService on a real engine: per face the dict of the host method on the same frame and location - streaming (BGR frames)
    and encode_face (an RGB image)"""
    engine = fresh_engine
    rng = np.random.default_rng(99)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 2, 192, 256, 4
    frames = _scene(rng, B, H, W)
    probe = engine.detect(frames, max_faces=K, det_thresh=1e-6)
    assert probe["counts"].min() >= 2
    thr = float(min(np.sort(probe["scores"][b, :probe["counts"][b]])[::-1][1] for b in range(B))) * 0.999
    calls = []
    inner = engine.face_quality
    engine.face_quality = lambda rects, rgb=False: calls.append((len(rects), rgb)) or inner(rects, rgb=rgb)
    fs, ref = FaceService(engine=engine), FaceService(engine=engine)
    out = fs.process_frames(frames, max_faces=K, det_thresh=thr, quality=True)
    plain = fs.process_frames(frames, max_faces=K, det_thresh=thr)
    n = 0
    for b in range(B):
        assert len(out[b]) == len(plain[b]) >= 2
        for f, p in zip(out[b], plain[b]):
            assert list(f.keys()) == list(p.keys()) + ["quality"] and f["bbox"] == p["bbox"]
            loc = box_to_location(f["bbox"], H, W)
            assert f["quality"] == ref.assess_face_quality(frames[b][..., ::-1], loc), (b, loc)
            n += 1
    assert calls and calls[0][1] is False and 1 <= calls[0][0] <= n and len(calls) == 1        # one device call for the batch
    rgb_img = np.ascontiguousarray(frames[0][..., ::-1])
    r = fs.encode_face(rgb_img, return_locations=True, return_quality=True)
    if r["success"]:
        assert r["quality"] == [ref.assess_face_quality(rgb_img, loc) for loc in r["locations"]]
        assert len(calls) == 2 and calls[1][1] is True
    else:
        assert r["message"] == "No faces detected in image"
