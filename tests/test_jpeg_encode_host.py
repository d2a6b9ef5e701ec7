"""CPU tests of the JPEG encoder's host side: frp_jpeg_encode_headers (needs only the built library, no GPU) against the segments of
PIL's file for the same geometry, quality, sampling and restart interval; mjpeg.multipart_part; the ABI list."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_model as M
from frp_amd import mjpeg, native
from test_jpeg_encode_model import content

CASES = [(h, w, q, ss, r) for (h, w) in ((16, 16), (17, 23), (33, 50), (1, 1))
         for q, ss, r in ((95, "4:2:0", 0), (75, "4:4:4", 0), (100, "4:2:0", 3), (30, "4:4:4", 1), (1, "4:2:0", 0), (50, "4:2:0", 65535))]
CASES.append((1080, 1920, 95, "4:2:0", 0))              # the workload's geometry, once


@pytest.mark.parametrize("h,w,q,ss,r", CASES)
def test_headers_equal_pils(h, w, q, ss, r):
    rr = r if r < 65535 else 0                              # (PIL's file for the DRI-less segments; the DRI payload is checked below)
    img = content("noise", h, w) if h * w <= 10000 else np.zeros((h, w, 3), np.uint8)
    pil = M.pil_encode(img, q, ss, rr)
    psegs, pscan = M.split_segments(pil)
    hdr = native.jpeg_encode_headers(w, h, q, ss, r)
    assert hdr[:2] == b"\xff\xd8"
    segs, rest = M.split_segments(hdr + b"\xff\xd9")
    assert rest == b""
    want_order = [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4] + ([0xDD] if r else []) + [0xDA]
    assert [m for m, _ in segs] == want_order
    for m in (0xDB, 0xC0, 0xC4, 0xDA) + ((0xDD,) if rr else ()):
        assert M.segments_of(segs, m) == M.segments_of(psegs, m), hex(m)
    if r:
        assert M.segments_of(segs, 0xDD) == [bytes([r >> 8, r & 255])]
    app0 = M.segments_of(segs, 0xE0)[0]
    assert app0[:5] == b"JFIF\0" and app0[5:7] == b"\x01\x01" and len(app0) == 14 and app0[12:] == b"\0\0"     # 1.01, no thumbnail
    if h * w <= 10000:
        # headers + the model's scan + EOI: a file PIL opens, with the pixels of PIL's own file
        info, coef, _ = M.forward(img, q, ss)
        ours = hdr + M.scan_bytes(info, coef, r) + b"\xff\xd9"
        a = np.asarray(Image.open(io.BytesIO(ours)).convert("RGB"))
        b = np.asarray(Image.open(io.BytesIO(pil)).convert("RGB"))
        assert a.shape == (h, w, 3) and np.array_equal(a, b)


def test_headers_refusals_write_nothing():
    lib = native.load_library()
    n = len(native.jpeg_encode_headers(40, 24, 95, "4:2:0", 0))
    assert len(native.jpeg_encode_headers(40, 24, 95, "4:2:0", 5)) == n + 6
    buf = np.full(n + 8, 0xA5, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.frp_jpeg_encode_headers(40, 24, 95, 420, 0, p, n - 1) == -1          # one byte short
    assert (buf == 0xA5).all()
    for args in ((0, 24, 95, 420, 0), (40, 0, 95, 420, 0), (65536, 24, 95, 420, 0), (40, 24, 0, 420, 0), (40, 24, 101, 420, 0),
                 (40, 24, 95, 422, 0), (40, 24, 95, 0, 0), (40, 24, 95, 420, -1), (40, 24, 95, 420, 65536)):
        assert lib.frp_jpeg_encode_headers(*args, p, buf.size) == -1, args
        assert (buf == 0xA5).all(), args
    assert lib.frp_jpeg_encode_headers(40, 24, 95, 420, 0, None, 4096) == -1
    assert lib.frp_jpeg_encode_headers(40, 24, 95, 420, 0, p, n) == n              # exactly enough
    assert (buf[n:] == 0xA5).all() and bytes(buf[:2]) == b"\xff\xd8"
    with pytest.raises(native.FrpError):
        native.jpeg_encode_headers(40, 24, 95, "4:2:2")


def test_multipart_part_round_trips_through_the_demuxer():
    frames = [M.pil_encode(content("noise", 24, 40, seed=s), 90) for s in range(3)]
    assert mjpeg.multipart_part(frames[0]) == b"--frame\r\nContent-Type: image/jpeg\r\n\r\n" + frames[0] + b"\r\n"
    body = b"".join(mjpeg.multipart_part(f) for f in frames)
    got = list(mjpeg.multipart_frames(io.BytesIO(body)))
    assert [bytes(g) for g in got] == frames


def test_new_symbols_are_part_of_the_abi():
    lib = native.load_library()
    for name in ("frp_jpeg_encode_headers", "frp_encode_jpeg", "frp_encode_jpeg_coefficients"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
    assert native.JPEG_SUBSAMPLING == {"4:2:0": 420, "4:4:4": 444}
