"""GPU tests of the encoder's optimised Huffman coding (FRP_FLAG_JPEG_OPTIMIZE: csrc/jpeg_encode_kernels.hip jpeg_enc_hist_kernel, the
per-image tables of the entropy stage, frp_encode_jpeg_histograms; Engine.encode_jpeg / encode_jpeg_enhanced(optimize=True)) and of the
service methods on top.  Integer arithmetic throughout: every comparison is exact - histograms element for element against the model
(tests/jpeg_optimize_model.py), files byte for byte against Pillow's save(optimize=True) AND against the model's file."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import enhance_model as EM
import jpeg_encode_model as M
import jpeg_optimize_model as OM
from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.face_service import FaceService
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

B, H, W = 3, 97, 131
OPT = native.FLAG_JPEG_OPTIMIZE


def _frames():
    """frame 0: uniform noise; frame 1: a smooth ramp with mild noise, a flat 16 x 16 patch at (8, 8) and, in the block at (32, 64), a
    faint 1-pixel checker - at low quality only its DC and coefficient 63 survive: a zero run of 62, three ZRL codes in front of one
    symbol; frame 2: flat patches, a noise band and a ramp (the model's mixed content)"""
    f = np.empty((B, H, W, 3), np.uint8)
    f[0] = OM._noise(31, H, W)
    f[1] = OM._smooth(32, H, W)
    f[1, 8:24, 8:24] = (70, 130, 200)
    yy, xx = np.mgrid[0:8, 0:8]
    f[1, 32:40, 64:72] = (128 + 20 * (1 - 2 * ((yy + xx) % 2)))[..., None]
    f[2] = OM._mixed(33, H, W)
    return f


FRAMES = _frames()
# a flat 8 x 8 crop, a 16 x 16 crop, a 33 x 50 noise crop, a smooth 40 x 72 crop, a whole frame: 3, 6, ... blocks - no multiple of
# the blocks a workgroup of any of the entropy kernels takes
MIXED = [(1, 10, 20, 18, 12), (2, 3, 21, 19, 5), (0, 40, 61, 73, 11), (1, 50, 100, 90, 28), (2, 0, W, H, 0)]
_WANT = {}


def _crop_rgb(rect, frames=FRAMES):
    b, top, right, bottom, left = rect
    return np.ascontiguousarray(frames[b, top:bottom, left:right, ::-1])


def _want(rgb, quality, ss, r=0):
    """Pillow's optimised file of `rgb`, computed once per input - and the model's, which has to be the same"""
    key = (rgb.shape, rgb.tobytes(), quality, ss, r)
    if key not in _WANT:
        pil = OM.pil_encode(rgb, quality, ss, r)
        assert OM.encode(rgb, quality, ss, r) == pil, ("model / Pillow", rgb.shape, quality, ss, r)
        _WANT[key] = pil
    return _WANT[key]


def _model_hist(rgb, quality, ss, r=0):
    info, coef, _ = M.forward(rgb, quality, ss)
    return OM.histogram(info, coef, r)


def _check(engine, rects, quality, ss, r=0, frames=FRAMES, rgb=False):
    """optimised files of `rects` against Pillow (and the model); on a mismatch the histogram says which half differs"""
    got = engine.encode_jpeg(rects, quality=quality, subsampling=ss, restart_mcus=r, rgb=rgb, optimize=True)
    assert len(got) == len(rects)
    for i, rect in enumerate(rects):
        crop = _crop_rgb(rect, frames)
        if rgb:
            crop = np.ascontiguousarray(crop[..., ::-1])
        ref = _want(crop, quality, ss, r)
        if got[i] != ref:
            dev = engine.encode_jpeg_histograms([rect], quality=quality, subsampling=ss, restart_mcus=r, rgb=rgb)[0]
            bad = np.flatnonzero(dev != _model_hist(crop, quality, ss, r))
            assert bad.size == 0, ("histogram", i, rect, bad[:8], dev[bad[:8]])
            gs, gscan = M.split_segments(got[i])
            rs, rscan = M.split_segments(ref)
            for m in (0xDB, 0xC0, 0xC4, 0xDD, 0xDA):
                assert M.segments_of(gs, m) == M.segments_of(rs, m), ("segment", hex(m), i, rect)
            assert gscan == rscan, ("scan", i, rect, len(gscan), len(rscan))
        assert got[i] == ref, ("file", i, rect, quality, ss, r)
    return got


@pytest.fixture()
def resident(engine):
    engine.upload_frames(FRAMES)
    return engine


def test_the_crops_are_what_the_list_says():
    flat8, c16, noise, smooth, whole = (_crop_rgb(r) for r in MIXED)
    assert flat8.shape == (8, 8, 3) and (flat8 == flat8[0, 0]).all()
    assert c16.shape == (16, 16, 3) and noise.shape == (33, 50, 3) and smooth.shape == (40, 72, 3) and whole.shape == (H, W, 3)
    for ss, per in (("4:2:0", 6), ("4:4:4", 3)):
        blocks = [per * M.geometry(c.shape[1], c.shape[0], ss)["mcus_x"] * M.geometry(c.shape[1], c.shape[0], ss)["mcus_y"] for c in (flat8, c16, noise, smooth, whole)]
        assert blocks[0] in (3, 6) and any(b % 4 for b in blocks) and sum(blocks[:4]) % 256 and sum(blocks[:2]) < 256      # a workgroup spans images
    # frame 1 at quality 20: a run of 62 zeros, coded as three ZRLs whose code is longer than Annex K's need not be (the lane's bits
    # come in two parts for that: ZRL codes of 16 bits, which no image here reaches, would not fit 64 together with the symbol)
    info, coef, _ = M.forward(_crop_rgb((1, 0, W, H, 0)), 20, "4:4:4")
    luma = coef[:info["mcus_x"] * info["mcus_y"] * 64].reshape(-1, 64)[:, np.asarray(M.ZIGZAG)]
    assert any(b[63] != 0 and not b[1:63].any() for b in luma)
    assert _model_hist(_crop_rgb((1, 0, W, H, 0)), 20, "4:4:4")[OM.AC0 + 0xF0] >= 3
    h = _model_hist(flat8, 85, "4:2:0")
    assert np.count_nonzero(h[OM.AC0:OM.AC0 + 256]) == 1 and h[OM.AC0] == 4      # one-symbol AC tables: the dummy blocks count too


@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
def test_histograms_equal_the_model(resident, ss):
    rects = MIXED + MIXED[::-1]
    for q, r in ((85, 0), (20, 3), (100, 1)):
        got = resident.encode_jpeg_histograms(rects, quality=q, subsampling=ss, restart_mcus=r)
        assert got.shape == (len(rects), native.JPEG_HIST_ELEMS) and got.dtype == np.uint32
        for i, rect in enumerate(rects):
            want = _model_hist(_crop_rgb(rect), q, ss, r)
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, (ss, q, r, i, rect, bad[:8], got[i][bad[:8]], want[bad[:8]])
    # the restart interval matters to the DC counts, and the entry alone agrees with the one inside a list
    a = resident.encode_jpeg_histograms(MIXED[4:], quality=20, subsampling=ss, restart_mcus=3)
    b = resident.encode_jpeg_histograms(MIXED[4:], quality=20, subsampling=ss)
    assert not np.array_equal(a[0, :32], b[0, :32]) and np.array_equal(a[0, 32:], b[0, 32:])


@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
def test_one_call_with_mixed_images(resident, ss):
    """small and large images in one index space: workgroups straddle images, and every image has tables of its own"""
    fwd = _check(resident, MIXED, 85, ss)
    rev = _check(resident, MIXED[::-1], 85, ss)
    assert rev == fwd[::-1]
    assert len({len(M.segments_of(M.split_segments(f)[0], 0xC4)[1]) for f in fwd}) > 1      # AC0 segments of different lengths
    for f, rect in zip(fwd, MIXED):
        assert [f] == resident.encode_jpeg([rect], quality=85, subsampling=ss, optimize=True), rect


@pytest.mark.parametrize("hw", [(1, 1), (9, 7), (17, 23)])
def test_geometries(resident, hw):
    h, w = hw
    rects = [(0, 0, w, h, 0), (2, H - h, W, H, W - w), (1, 30, 40 + w, 30 + h, 40)]
    for ss in ("4:2:0", "4:4:4"):
        _check(resident, rects, 90, ss)


@pytest.mark.parametrize("quality", [100, 85, 20])
def test_qualities(resident, quality):
    for ss in ("4:2:0", "4:4:4"):
        _check(resident, [(b, 0, W, H, 0) for b in range(B)] + MIXED[2:4], quality, ss)


@pytest.mark.parametrize("r", [1, 3])
def test_restart_intervals(resident, r):
    for ss, q in (("4:2:0", 85), ("4:4:4", 20)):
        got = _check(resident, MIXED, q, ss, r)
        assert b"\xff\xd0" in got[4] and b"\xff\xd7" in got[4]                  # more than 8 intervals in the whole frame
        assert native.jpeg_info(got[4])["restart_interval"] == r


def test_rgb_flag(resident):
    rects = MIXED[2:]
    as_rgb = _check(resident, rects, 85, "4:2:0", rgb=True)
    plain = _check(resident, rects, 85, "4:2:0")
    assert all(a != b for a, b in zip(as_rgb, plain))


def _pil_file(rgb, quality, ss="4:2:0", **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=M.PIL_SUBSAMPLING[ss], **kw)
    return buf.getvalue()


def test_enhanced_route(resident):
    """services/enhancer.py:64-92 with Pillow on the host, optimize=True included: an upscaled crop and one that keeps its size"""
    jobs = [((0, 20, 80, 70, 10), (99, 71)), ((2, 40, 81, 73, 40), (41, 33)), ((1, 0, W, H, 0), (2 * W, 2 * H))]
    rects, sizes = [r for r, _ in jobs], [s for _, s in jobs]
    for ss in ("4:2:0", "4:4:4"):
        got = resident.encode_jpeg_enhanced(rects, sizes, quality=85, subsampling=ss, optimize=True)
        plain = resident.encode_jpeg_enhanced(rects, sizes, quality=85, subsampling=ss)
        for i, (r, s) in enumerate(jobs):
            enhanced = EM.pillow_enhance(_crop_rgb(r), *s)
            assert got[i] == _pil_file(enhanced, 85, ss, optimize=True), (ss, i)
            assert got[i] == _want(enhanced, 85, ss), (ss, i)
            assert plain[i] == _pil_file(enhanced, 85, ss), (ss, i)
    assert resident.encode_jpeg_enhanced(rects[:1], sizes[:1], quality=85, restart_mcus=3, optimize=True)[0] == \
        _want(EM.pillow_enhance(_crop_rgb(rects[0]), *sizes[0]), 85, "4:2:0", 3)
    as_rgb = resident.encode_jpeg_enhanced(rects[:2], sizes[:2], quality=85, rgb=True, optimize=True)
    for i in range(2):
        assert as_rgb[i] == _want(EM.pillow_enhance(np.ascontiguousarray(_crop_rgb(rects[i])[..., ::-1]), *sizes[i]), 85, "4:2:0"), i


def test_service(resident, monkeypatch):
    for k in ("ENHANCER_UPSCALE_FACTOR", "ENHANCER_MAX_PIXELS", "ENHANCER_JPEG_QUALITY", "ENHANCER_SHARPEN"):
        monkeypatch.delenv(k, raising=False)
    fs = FaceService(engine=resident)

    def enhanced(bgr, quality, optimize):
        h, w = bgr.shape[:2]
        return _pil_file(EM.pillow_enhance(np.ascontiguousarray(bgr[..., ::-1]), *EM.enhanced_size(w, h)), quality, optimize=optimize)

    # the reference's own file: x2, UnsharpMask(1, 120, 3), quality 85, optimize=True
    snap = fs.enhance_snapshot(0, optimize=True)
    assert snap == enhanced(FRAMES[0], 85, True) and Image.open(io.BytesIO(snap)).size == (2 * W, 2 * H)
    assert fs.enhance_snapshot(0) == enhanced(FRAMES[0], 85, False)               # the default: as before
    assert fs.snapshot_jpeg(1, quality=80, optimize=True) == _want(_crop_rgb((1, 0, W, H, 0)), 80, "4:2:0")
    assert fs.snapshot_jpeg(1, quality=80) == M.pil_encode(_crop_rgb((1, 0, W, H, 0)), 80)
    assert fs.snapshot_jpeg(2, quality=70, enhance=True, optimize=True) == enhanced(FRAMES[2], 70, True)
    assert fs.encode_frames(quality=70, optimize=True) == [_want(_crop_rgb((b, 0, W, H, 0)), 70, "4:2:0") for b in range(B)]
    assert fs.encode_frames(quality=70) == [M.pil_encode(_crop_rgb((b, 0, W, H, 0)), 70) for b in range(B)]
    faces = [(0, (10, 50, 40, 20)), (1, (-5, 125, 30, 95)), (2, (50, 20, 70, 0))]
    crops = [FRAMES[0, 0:55, 5:65], FRAMES[1, 0:48, 80:W], FRAMES[2, 40:80, 0:30]]
    thumbs = fs.face_thumbnails(faces, margin=0.5, quality=90, optimize=True)
    assert thumbs == [_want(np.ascontiguousarray(c[..., ::-1]), 90, "4:2:0") for c in crops]
    assert fs.face_thumbnails(faces, margin=0.5, quality=90) == [M.pil_encode(np.ascontiguousarray(c[..., ::-1]), 90) for c in crops]
    assert fs.face_thumbnails(faces, margin=0.5, quality=90, enhance=True, optimize=True) == [enhanced(c, 90, True) for c in crops]
    assert fs.snapshot_jpeg(9, optimize=True) is None and fs.face_thumbnails([(5, (0, 10, 10, 0))], optimize=True) == []      # logged, not raised


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(eng, rects, n, q, ss, r, flags, out, cap, offsets):
    rr = np.ascontiguousarray(rects, np.int32)
    return eng._lib.frp_encode_jpeg(eng._h, _p(rr), n, q, ss, r, flags, _p(out), cap, _p(offsets))


def test_contract(resident):
    engine = resident
    good = (0, 2, 40, 30, 4)
    ref = _want(_crop_rgb(good), 95, "4:2:0")
    size = len(ref)
    assert engine.encode_jpeg([good], optimize=True) == [ref]
    out = np.full(2 * size + 4096, 0xA5, np.uint8)
    offsets = np.full(3, -7, np.int64)
    # too small by one byte: refused, sizes reported, nothing written; exactly enough goes through
    assert _raw(engine, [good, good], 2, 95, 420, 0, OPT, out, 2 * size - 1, offsets) == -1
    assert offsets.tolist() == [0, size, 2 * size] and (out == 0xA5).all()
    assert _raw(engine, [good, good], 2, 95, 420, 0, OPT, out, 2 * size, offsets) == 0
    assert out[:2 * size].tobytes() == ref + ref and (out[2 * size:] == 0xA5).all()
    # n == 0
    out[:] = 0xA5
    offsets[:] = -7
    assert _raw(engine, [good], 0, 95, 420, 0, OPT, out, out.size, offsets) == 0 and offsets[0] == 0 and (out == 0xA5).all()
    assert engine.encode_jpeg(np.zeros((0, 5), np.int32), optimize=True) == []
    assert engine.encode_jpeg_histograms(np.zeros((0, 5), np.int32)).shape == (0, native.JPEG_HIST_ELEMS)
    # the flag next to FRP_FLAG_RGB is accepted, next to any other refused
    offsets[:] = -7
    assert _raw(engine, [good], 1, 95, 420, 0, OPT | native.FLAG_RGB, out, out.size, offsets) == 0
    out[:] = 0xA5
    offsets[:] = -7
    for flags in (OPT | native.FLAG_FORCED_K, OPT | native.FLAG_NO_MATCH, OPT | (1 << 31), OPT << 1):
        assert _raw(engine, [good], 1, 95, 420, 0, flags, out, out.size, offsets) == -1, flags
        assert (out == 0xA5).all() and (offsets == -7).all()
    # the other arguments are checked as without the flag
    for q, ss, r in [(0, 420, 0), (101, 420, 0), (95, 422, 0), (95, 420, -1), (95, 420, 65536)]:
        assert _raw(engine, [good], 1, q, ss, r, OPT, out, out.size, offsets) == -1, (q, ss, r)
    assert _raw(engine, [good, (B, 2, 40, 30, 4)], 2, 95, 420, 0, OPT, out, out.size, offsets) == -1
    assert b"rectangle 1 " in engine._lib.frp_last_error(engine._h)
    assert (out == 0xA5).all() and (offsets == -7).all()
    # the coefficient, pixel and quality entry points refuse the flag with nothing written
    rr = np.ascontiguousarray([good], np.int32)
    coef = np.full(2 * 3 * 6 * 64, 0x5A5A, np.int16)                              # good is 36 x 28: 3 x 2 MCUs at 4:2:0
    for flags in (OPT, OPT | native.FLAG_RGB):
        assert engine._lib.frp_encode_jpeg_coefficients(engine._h, _p(rr), 1, 95, 420, flags, _p(coef), coef.size) == -1
        assert (coef == 0x5A5A).all()
        sz = np.ascontiguousarray([(72, 56)], np.int32)
        prm = native.FrpEnhanceParams(1.0, 120, 3, 1)
        px = np.full(3 * 72 * 56, 0xA5, np.uint8)
        assert engine._lib.frp_enhance_pixels(engine._h, _p(rr), _p(sz), 1, C.byref(prm), flags, _p(px), px.size, _p(offsets)) == -1
        assert (px == 0xA5).all() and (offsets == -7).all()
        sums = np.full(4, -7, np.int64)
        assert engine._lib.frp_face_quality(engine._h, _p(rr), 1, flags, _p(sums)) == -1
        assert (sums == -7).all()
    assert engine._lib.frp_encode_jpeg_coefficients(engine._h, _p(rr), 1, 95, 420, 0, _p(coef), coef.size) == 0
    # the histogram entry checks its size, and writes nothing when it refuses
    hist = np.full(2 * native.JPEG_HIST_ELEMS, 0xA5A5A5A5, np.uint32)
    for elems in (native.JPEG_HIST_ELEMS - 1, 2 * native.JPEG_HIST_ELEMS):
        assert engine._lib.frp_encode_jpeg_histograms(engine._h, _p(rr), 1, 95, 420, 0, 0, _p(hist), elems) == -1
    assert engine._lib.frp_encode_jpeg_histograms(engine._h, _p(rr), 1, 95, 420, 0, native.FLAG_NO_MATCH, _p(hist), native.JPEG_HIST_ELEMS) == -1
    assert (hist == 0xA5A5A5A5).all()
    with pytest.raises(FrpError):
        engine.encode_jpeg([good], quality=0, optimize=True)
    # the Python wrapper retries once with the reported size: noise at quality 100 is larger than its first guess
    big = engine.encode_jpeg([(0, 0, W, H, 0)] * 3, quality=100, subsampling="4:4:4", optimize=True)
    assert big[0] == big[2] == _want(_crop_rgb((0, 0, W, H, 0)), 100, "4:4:4")


def _scene(rng, n, h, w):
    base = rng.integers(0, 255, size=(n, h // 16, w // 16, 3)).astype(np.float32)
    base = np.repeat(np.repeat(base, 16, axis=1), 16, axis=2)
    return np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)


def test_results_of_the_last_pass_stay_fetchable(fresh_engine):
    engine = fresh_engine
    rng = np.random.default_rng(12)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    n, h, w, K = 2, 192, 256, 6
    frames = _scene(rng, n, h, w)
    engine.gallery_set(rng.standard_normal((300, 512)).astype(np.float32))
    engine.upload_frames(frames)
    engine.process_resident(K, flags=native.FLAG_FORCED_K)
    rects = [(1, 17, 200, 99, 31), (0, 0, w, h, 0)]
    queued = engine.encode_jpeg(rects, quality=90, optimize=True)      # queued behind the pending pass, before anything was fetched
    assert queued == [_want(_crop_rgb(r, frames), 90, "4:2:0") for r in rects]
    before = engine.fetch_results()
    assert before["counts"].tolist() == [K] * n
    assert engine.encode_jpeg(rects, quality=90, optimize=True) == queued
    assert engine.encode_jpeg_enhanced(rects[:1], [(338, 164)], optimize=True)[0] == \
        _want(EM.pillow_enhance(_crop_rgb(rects[0], frames), 338, 164), 85, "4:2:0")
    hist = engine.encode_jpeg_histograms(rects[:1], quality=90)
    assert np.array_equal(hist[0], _model_hist(_crop_rgb(rects[0], frames), 90, "4:2:0"))
    after = engine.fetch_results()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


def test_determinism_and_file_sizes(resident):
    rects = MIXED + [(b, 0, W, H, 0) for b in range(B)] + [(0, 0, 1, 1, 0), (1, 10, 20, 18, 12)]
    for ss in ("4:2:0", "4:4:4"):
        for q in (85, 20):
            a = resident.encode_jpeg(rects, quality=q, subsampling=ss, optimize=True)
            b = resident.encode_jpeg(rects, quality=q, subsampling=ss, optimize=True)
            assert a == b
            plain = resident.encode_jpeg(rects, quality=q, subsampling=ss)
            for rect, fo, fp in zip(rects, a, plain):
                so, sp = M.split_segments(fo), M.split_segments(fp)
                assert len(so[1]) <= len(sp[1]), (rect, ss, q)                 # the scan never grows ...
                for m in (0xE0, 0xDB, 0xC0, 0xDA):
                    assert M.segments_of(so[0], m) == M.segments_of(sp[0], m)
                if (rect[3] - rect[1]) * (rect[2] - rect[4]) >= 16 * 16 * 4:
                    assert len(fo) <= len(fp), (rect, ss, q)                    # ... and neither does the file, tiny images apart
                assert np.array_equal(native.jpeg_coefficients(fo)[1], native.jpeg_coefficients(fp)[1]), rect
