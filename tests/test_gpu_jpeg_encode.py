"""GPU tests of the JPEG encoder (csrc/jpeg_encode_kernels.hip, frp_encode_jpeg, Engine.encode_jpeg) and of the service methods on top
of it.  Integer arithmetic throughout: every comparison is exact - files byte for byte against PIL / libjpeg (or the golden files PIL
wrote, for restart intervals), coefficients element for element against the numpy model (tests/jpeg_encode_model.py)."""
import ctypes as C
import glob
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_model as M
from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.face_service import FaceService
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ZZ = np.asarray(M.ZIGZAG)


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _whole(frames):
    B, H, W, _ = frames.shape
    return [(b, 0, W, H, 0) for b in range(B)]


def _crop_rgb(frames_bgr, rect):
    b, top, right, bottom, left = rect
    return np.ascontiguousarray(frames_bgr[b, top:bottom, left:right, ::-1])


def _check_files(engine, frames_bgr, rects, quality, ss, r=0, want=None):
    """files of `rects` against PIL of the numpy crops (or `want`); on a mismatch the coefficients say which half differs"""
    got = engine.encode_jpeg(rects, quality=quality, subsampling=ss, restart_mcus=r)
    assert len(got) == len(rects)
    for i, rect in enumerate(rects):
        rgb = _crop_rgb(frames_bgr, rect)
        ref = want[i] if want is not None else M.pil_encode(rgb, quality, ss, r)
        if got[i] != ref:
            info, coef, _ = M.forward(rgb, quality, ss)
            dev = engine.encode_jpeg_coefficients([rect], quality=quality, subsampling=ss)
            bad = np.flatnonzero(dev != coef)
            assert bad.size == 0, ("coefficients", rect, quality, ss, bad[:8], dev[bad[:8]], coef[bad[:8]])
            gs, gscan = M.split_segments(got[i])
            rs, rscan = M.split_segments(ref)
            for m in (0xDB, 0xC0, 0xC4, 0xDD, 0xDA):
                assert M.segments_of(gs, m) == M.segments_of(rs, m), ("segment", hex(m), rect)
            n = min(len(gscan), len(rscan))
            first = next((k for k in range(n) if gscan[k] != rscan[k]), n)
            assert gscan == rscan, ("scan", rect, quality, ss, r, len(gscan), len(rscan), first, gscan[first:first + 8].hex(), rscan[first:first + 8].hex())
            assert got[i] == ref, ("file", rect)
    return got


def _composite():
    """two 40 x 72 BGR frames: 8 x 8 black / white checker, 1-pixel checker, uniform noise, a flat patch | Gaussian noise"""
    rng = np.random.default_rng(2024)
    f0 = np.zeros((40, 72, 3), np.uint8)
    yy, xx = np.mgrid[0:40, 0:72]
    f0[:, 0:24] = ((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)[:, 0:24, None]
    f0[:, 24:40] = (((yy + xx) % 2) * 255).astype(np.uint8)[:, 24:40, None]
    f0[:, 40:56] = rng.integers(0, 256, size=(40, 16, 3), dtype=np.uint8)
    f0[:, 56:72] = (70, 130, 200)
    f1 = np.clip(rng.normal(128, 30, size=(40, 72, 3)), 0, 255).astype(np.uint8)
    return np.stack([f0, f1])


def _blocks(info, coef):
    """-> per component [blocks, 64] in zig-zag order"""
    out, off = [], 0
    for c in range(3):
        n = info["mcus_x"] * info["h_samp"][c] * info["mcus_y"] * info["v_samp"][c]
        out.append(coef[off:off + n * 64].reshape(n, 64)[:, ZZ].astype(np.int64))
        off += n * 64
    return out


def _max_zero_run(zz):
    """longest zero run that ENDS in a non-zero AC coefficient (trailing zeros are EOB, not ZRL)"""
    best, prev = 0, 0
    for k in np.flatnonzero(zz[1:]) + 1:
        best = max(best, k - prev - 1)
        prev = k
    return best


def _assert_special_symbols(frames):
    """on the reference alone, before the device is asked: a luma DC difference of category 11, a block without EOB, an AC-free
    block, a zero run >= 16 and a stuffed byte"""
    rgb0, rgb1 = _crop_rgb(frames, (0, 0, 72, 40, 0)), _crop_rgb(frames, (1, 0, 72, 40, 0))
    info, coef, _ = M.forward(rgb0, 100, "4:4:4")
    y = _blocks(info, coef)[0]
    grid = y[:, 0].reshape(info["mcus_y"], info["mcus_x"])
    assert np.abs(np.diff(grid, axis=1)).max() >= 1024                      # scan order at 4:4:4: along the block row
    assert (y[:, 63] != 0).any()
    assert (np.abs(y[:, 1:]).sum(axis=1) == 0).any()
    info1, coef1, _ = M.forward(rgb1, 50, "4:2:0")
    assert max(_max_zero_run(b) for comp in _blocks(info1, coef1) for b in comp) >= 16
    _, scan = M.split_segments(M.pil_encode(rgb0, 100, "4:4:4"))
    assert b"\xff\x00" in scan


def test_composite_inputs_exercise_the_special_symbols():
    _assert_special_symbols(_composite())


@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("quality", [100, 95, 50])
def test_composite_frames(engine, quality, ss):
    frames = _composite()
    _assert_special_symbols(frames)
    engine.upload_frames(frames)
    rects = _whole(frames)
    want = np.concatenate([M.forward(_crop_rgb(frames, r), quality, ss)[1] for r in rects])
    got = engine.encode_jpeg_coefficients(rects, quality=quality, subsampling=ss)
    assert got.dtype == np.int16 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    _check_files(engine, frames, rects, quality, ss)


@pytest.mark.parametrize("hw", [(1, 1), (9, 7), (17, 23), (24, 40), (33, 50)])
def test_edge_geometries(engine, hw):
    frames = _noise(hw[0] * 100 + hw[1], (2,) + hw + (3,))
    engine.upload_frames(frames)
    for ss in ("4:2:0", "4:4:4"):
        rects = _whole(frames)
        want = np.concatenate([M.forward(_crop_rgb(frames, r), 90, ss)[1] for r in rects])
        assert np.array_equal(engine.encode_jpeg_coefficients(rects, quality=90, subsampling=ss), want), ss
        _check_files(engine, frames, rects, 90, ss)


def test_crops_of_several_sizes_from_three_frames(engine):
    frames = _noise(5, (3, 64, 96, 3))
    frames[1] = (frames[1].astype(np.int32) // 4 + np.arange(96)[None, :, None] * 2).astype(np.uint8)      # smoother: other code lengths
    engine.upload_frames(frames)
    rects = [(0, 1, 18, 18, 1), (2, 3, 96, 64, 45), (1, 7, 60, 40, 11), (0, 63, 96, 64, 95), (1, 0, 96, 64, 0), (2, 5, 14, 55, 13),
             (1, 9, 80, 10, 3), (2, 31, 64, 47, 33), (1, 7, 60, 40, 11)]
    for ss, q in (("4:2:0", 95), ("4:4:4", 80)):
        got = _check_files(engine, frames, rects, q, ss)
        assert got[2] == got[8]
        # the raw entry: offsets and the files back to back
        r = np.ascontiguousarray(rects, np.int32)
        offsets = np.zeros(len(rects) + 1, np.int64)
        out = np.zeros(sum(map(len, got)), np.uint8)
        rc = engine._lib.frp_encode_jpeg(engine._h, r.ctypes.data_as(C.c_void_p), len(rects), q, native.JPEG_SUBSAMPLING[ss], 0, 0,
                                         out.ctypes.data_as(C.c_void_p), out.size, offsets.ctypes.data_as(C.c_void_p))
        assert rc == 0
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in got])]).tolist()
        assert out.tobytes() == b"".join(got)


def _golden():
    out = []
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "jpeg_encode", "*.npz"))):
        z = np.load(path)
        out.append((os.path.basename(path)[:-4], z["rgb"], z["jpeg"].tobytes(), int(z["quality"]), str(z["subsampling"]), int(z["restart_mcus"])))
    return out


GOLDEN = _golden()


@pytest.mark.parametrize("name", [g[0] for g in GOLDEN])
def test_restart_intervals_equal_the_golden_files(engine, name):
    _, rgb, jpeg, q, ss, r = next(g for g in GOLDEN if g[0] == name)
    assert r > 0
    if name.startswith(("r1_", "r3_444")):
        assert b"\xff\xd0" in jpeg[jpeg.index(b"\xff\xd7"):]                 # more than 8 intervals: RST0 again behind RST7
    frames = np.ascontiguousarray(rgb[None, :, :, ::-1])
    engine.upload_frames(frames)
    _check_files(engine, frames, _whole(frames), q, ss, r, want=[jpeg])


def test_golden_set_covers_both_intervals_and_the_marker_wrap():
    rs = {g[5] for g in GOLDEN}
    assert {1, 3} <= rs and len(GOLDEN) >= 4
    for name, rgb, jpeg, q, ss, r in GOLDEN:
        assert rgb.shape[0] <= 48 and rgb.shape[1] <= 72
        info = M.geometry(rgb.shape[1], rgb.shape[0], ss)
        if name.startswith("r1_"):
            assert info["mcus_x"] * info["mcus_y"] > 8


def test_rgb_flag_equals_the_swapped_frame(engine):
    frames = _noise(8, (2, 24, 40, 3))
    rects = _whole(frames) + [(1, 3, 30, 20, 5)]
    engine.upload_frames(frames)
    as_rgb = engine.encode_jpeg(rects, quality=85, rgb=True)
    plain = engine.encode_jpeg(rects, quality=85)
    engine.upload_frames(np.ascontiguousarray(frames[..., ::-1]))
    assert engine.encode_jpeg(rects, quality=85) == as_rgb
    assert all(a != b for a, b in zip(as_rgb, plain))
    for rect, f in zip(rects, as_rgb):
        b, top, right, bottom, left = rect
        assert f == M.pil_encode(np.ascontiguousarray(frames[b, top:bottom, left:right]), 85)


def _raw(eng, rects, n, q, ss, r, flags, out, cap, offsets):
    rr = np.ascontiguousarray(rects, np.int32)
    return eng._lib.frp_encode_jpeg(eng._h, rr.ctypes.data_as(C.c_void_p), n, q, ss, r, flags, out.ctypes.data_as(C.c_void_p), cap,
                                    offsets.ctypes.data_as(C.c_void_p))


def test_refusals_leave_out_untouched(engine, fresh_engine):
    frames = _noise(9, (2, 33, 50, 3))
    B, H, W, _ = frames.shape
    engine.upload_frames(frames)
    good = (1, 2, 40, 30, 4)
    size = len(engine.encode_jpeg([good])[0])
    out = np.full(2 * size + 4096, 0xA5, np.uint8)
    offsets = np.full(3, -7, np.int64)
    for rect in [(-1, 2, 40, 30, 4), (B, 2, 40, 30, 4), (1, -1, 40, 30, 4), (1, 30, 40, 30, 4), (1, 2, 40, H + 1, 4), (1, 2, 40, 30, -1),
                 (1, 2, 40, 30, 40), (1, 2, W + 1, 30, 4)]:
        assert _raw(engine, [good, rect], 2, 95, 420, 0, 0, out, out.size, offsets) == -1, rect
        assert b"rectangle 1 " in engine._lib.frp_last_error(engine._h)
        assert (out == 0xA5).all(), rect
        with pytest.raises(FrpError):
            engine.encode_jpeg([rect])
    for q, ss, r, flags in [(0, 420, 0, 0), (101, 420, 0, 0), (95, 422, 0, 0), (95, 0, 0, 0), (95, 420, -1, 0), (95, 420, 65536, 0),
                            (95, 420, 0, native.FLAG_FORCED_K), (95, 420, 0, native.FLAG_RGB | native.FLAG_NO_MATCH), (95, 420, 0, 1 << 31)]:
        assert _raw(engine, [good], 1, q, ss, r, flags, out, out.size, offsets) == -1, (q, ss, r, flags)
        assert (out == 0xA5).all()
    assert _raw(engine, [good], -1, 95, 420, 0, 0, out, out.size, offsets) == -1
    assert _raw(fresh_engine, [good], 1, 95, 420, 0, 0, out, out.size, offsets) == -1
    assert b"no resident frames" in fresh_engine._lib.frp_last_error(fresh_engine._h)
    assert (out == 0xA5).all()
    # too small by one byte: refused, sizes reported, nothing written
    offsets[:] = -7
    assert _raw(engine, [good, good], 2, 95, 420, 0, 0, out, 2 * size - 1, offsets) == -1
    assert offsets.tolist() == [0, size, 2 * size] and (out == 0xA5).all()
    # n == 0
    offsets[:] = -7
    assert _raw(engine, [good], 0, 95, 420, 0, 0, out, out.size, offsets) == 0 and offsets[0] == 0 and (out == 0xA5).all()
    assert engine.encode_jpeg(np.zeros((0, 5), np.int32)) == []
    # ... and exactly enough goes through
    assert _raw(engine, [good, good], 2, 95, 420, 0, 0, out, 2 * size, offsets) == 0
    ref = M.pil_encode(_crop_rgb(frames, good), 95)
    assert out[:2 * size].tobytes() == ref + ref and (out[2 * size:] == 0xA5).all()
    # the Python wrapper retries once with the reported size: noise at quality 100 is larger than its first guess
    big = engine.encode_jpeg([(0, 0, W, H, 0)] * 3, quality=100, subsampling="4:4:4")
    assert big[0] == M.pil_encode(_crop_rgb(frames, (0, 0, W, H, 0)), 100, "4:4:4") and big[0] == big[2]


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
    rects = [(1, 17, 200, 99, 31), (0, 0, W, H, 0)]
    queued = engine.encode_jpeg(rects, quality=90)                    # queued behind the pending pass, before anything was fetched
    assert queued == [M.pil_encode(_crop_rgb(frames, r), 90) for r in rects]
    before = engine.fetch_results()
    assert before["counts"].tolist() == [K] * B
    assert engine.encode_jpeg(rects, quality=90) == queued
    after = engine.fetch_results()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


def test_round_trip_through_the_device_decoder(fresh_engine):
    """(h) files written with r = 8 go back in through upload_jpeg_async + swap_frames: 4 frames x 16 intervals, enough for the device
    entropy decoder to take the batch; the resident pixels are PIL's decode of the files"""
    engine = fresh_engine
    frames = _scene(np.random.default_rng(88), 4, 128, 256)
    engine.upload_frames(frames)
    files = engine.encode_jpeg(_whole(frames), quality=90, restart_mcus=8)
    for f in files:
        assert native.jpeg_info(f)["restart_interval"] == 8 and f.count(b"\xff\xd7") >= 1
    n0 = engine.jpeg_device_batches()
    engine.upload_jpeg_async(files)
    engine.swap_frames()
    assert engine.jpeg_device_batches() == n0 + 1
    got = engine.det_source()
    want = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., ::-1] for f in files])
    assert np.array_equal(got, want)


def test_two_1080p_frames(engine):
    """(i) the workload's own geometry: 2 x 48960 blocks, bit offsets past 2^23, against PIL's bytes"""
    rng = np.random.default_rng(1080)
    frames = _scene(rng, 2, 1088, 1920)[:, :1080]
    frames = np.ascontiguousarray(frames)
    engine.upload_frames(frames)
    got = engine.encode_jpeg(_whole(frames), quality=95)
    for b in range(2):
        ref = M.pil_encode(np.ascontiguousarray(frames[b, :, :, ::-1]), 95)
        assert len(got[b]) == len(ref) and got[b] == ref, b


def test_service_snapshot_and_thumbnails(engine):
    frames = _noise(21, (2, 64, 96, 3))
    engine.upload_frames(frames)
    fs = FaceService(engine=engine)
    snap = fs.snapshot_jpeg(1, quality=80)
    assert snap == M.pil_encode(np.ascontiguousarray(frames[1, :, :, ::-1]), 80)
    im = Image.open(io.BytesIO(snap))
    assert im.size == (96, 64)
    every = fs.encode_frames(quality=70)
    assert [Image.open(io.BytesIO(f)).size for f in every] == [(96, 64)] * 2
    faces = [(0, (10, 50, 40, 20)), (1, (-5, 110, 30, 80)), (1, (50, 20, 70, 0))]
    thumbs = fs.face_thumbnails(faces, margin=0.5, quality=90)
    sizes = [Image.open(io.BytesIO(t)).size for t in thumbs]
    assert sizes == [(60, 55), (31, 48), (30, 24)]                          # (w, h): grown by half, clipped at the frame border
    assert thumbs[0] == M.pil_encode(np.ascontiguousarray(frames[0, 0:55, 5:65, ::-1]), 90)
    assert fs.face_thumbnails([(5, (0, 10, 10, 0))]) == [] and fs.snapshot_jpeg(9) is None      # logged, not raised
