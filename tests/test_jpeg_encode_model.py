"""CPU: the numpy model of the JPEG encoder (tests/jpeg_encode_model.py) against PIL / libjpeg - quantised coefficients element for
element (PIL's file decoded by oracle.jpeg.huffman_decode) and the entropy-coded segment byte for byte."""
import numpy as np
import pytest

import jpeg_encode_model as M
from oracle.jpeg import huffman_decode

SIZES = [(16, 16), (24, 40), (17, 23), (33, 50), (64, 48), (9, 7), (40, 24), (8, 100), (1, 1), (50, 34), (20, 36)]      # (H, W)
QUALITIES = [95, 75, 100, 30]


def content(kind, h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(3 * xx + yy) % 256, (2 * yy + 40) % 256, (xx + 2 * yy + 90) % 256], -1).astype(np.uint8)
    return (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("kind", ["noise", "ramp", "binary"])
def test_model_equals_pil(kind, subsampling):
    for h, w in SIZES:
        img = content(kind, h, w)
        for q in QUALITIES:
            info, coef, qt = M.forward(img, q, subsampling)
            for r in (0, 1, 3):
                data = M.pil_encode(img, q, subsampling, r)
                pinfo, pcoef, pq = huffman_decode(data)
                tag = (kind, h, w, q, subsampling, r)
                assert all(pinfo[k] == info[k] for k in info), tag
                assert pinfo["restart_interval"] == r, tag
                assert np.array_equal(pq[0], qt[0]) and np.array_equal(pq[1], qt[1]) and np.array_equal(pq[2], qt[1]), tag
                bad = np.flatnonzero(pcoef != coef)
                assert bad.size == 0, (tag, bad[:4], pcoef[bad[:4]], coef[bad[:4]])
                segs, scan = M.split_segments(data)
                assert M.scan_bytes(info, coef, r) == scan, tag


def test_segment_splitter_and_tables():
    data = M.pil_encode(content("noise", 24, 40), 75, "4:2:0", 3)
    segs, scan = M.split_segments(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    dht = M.segments_of(segs, 0xC4)
    want = [bytes([0x00] + M.DC_BITS[0] + M.DC_VALS[0]), bytes([0x10] + M.AC_BITS[0] + M.AC_VALS[0]),
            bytes([0x01] + M.DC_BITS[1] + M.DC_VALS[1]), bytes([0x11] + M.AC_BITS[1] + M.AC_VALS[1])]
    assert dht == want
    qt = M.quant_tables(75)
    assert M.segments_of(segs, 0xDB) == [bytes([t]) + bytes(int(qt[t][z]) for z in M.ZIGZAG) for t in (0, 1)]
    assert data.endswith(scan + b"\xff\xd9")
