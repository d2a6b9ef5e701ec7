"""CPU model of the baseline JPEG ENCODER (TEST INFRASTRUCTURE, like tests/quality_model.py: imported by tests/ only; the product path is
csrc/jpeg_encode_kernels.hip + csrc/jpeg_encode_api.cpp).

The forward pipeline of libjpeg at its defaults, restated in numpy from the published IJG definitions: jccolor.c (16-bit fixed-point
RGB -> YCbCr), jcsample.c (h2v2 box filter with the alternating 1, 2 bias; edge replication before and after), jfdctint.c (LL&M forward
DCT, 13-bit constants, two passes), jcdctmgr.c (quantisation by division with rounding away from zero at one half), jccoefct.c (dummy
blocks of partial MCUs), plus a plain ITU-T T.81 Annex F sequential Huffman scan writer (Annex K.3 tables) and a segment splitter.
PINNED: tests/test_jpeg_encode_model.py holds it to PIL's coefficients and scan bytes, bit for bit.

Coefficient layout = frp_jpeg_coefficients': per component [blocks_y][blocks_x][64] int16 in natural order over the MCU-padded grid,
components back to back.
"""
from __future__ import annotations

import numpy as np

from oracle.jpeg import (CONST_BITS, PASS1_BITS, F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602,
                         F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026, _ZIGZAG)

ZIGZAG = list(_ZIGZAG)

# Annex K.1 / K.2, natural order
K1_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
K2_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)

# Annex K.3: (BITS[16], HUFFVAL) of the DC / AC tables for luminance (0) and chrominance (1)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = ([
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

SAMPLINGS = {"4:2:0": (2, 2), "4:4:4": (1, 1)}      # luma factors; chroma is 1 x 1
PIL_SUBSAMPLING = {"4:2:0": 2, "4:4:4": 0}


def quant_tables(quality: int) -> np.ndarray:
    """[2, 64] natural order: libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (K1_LUMA, K2_CHROMA)])


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb: np.ndarray):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_right(p, width):
    return p if p.shape[1] >= width else np.concatenate([p, np.repeat(p[:, -1:], width - p.shape[1], axis=1)], axis=1)


def _pad_bottom(p, height):
    return p if p.shape[0] >= height else np.concatenate([p, np.repeat(p[-1:], height - p.shape[0], axis=0)], axis=0)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(v, first):
    """one LL&M pass over the LAST axis (jfdctint.c)"""
    d = [v[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    o[0] = (tmp10 + tmp11) << PASS1_BITS if first else _descale(tmp10 + tmp11, PASS1_BITS)
    o[4] = (tmp10 - tmp11) << PASS1_BITS if first else _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * F_0_541196100
    o[2] = _descale(z1 + tmp13 * F_0_765366865, sh)
    o[6] = _descale(z1 + tmp12 * (-F_1_847759065), sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F_1_175875602
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F_0_298631336, tmp5 * F_2_053119869, tmp6 * F_3_072711026, tmp7 * F_1_501321110
    z1, z2 = z1 * (-F_0_899976223), z2 * (-F_2_562915447)
    z3, z4 = z3 * (-F_1_961570560) + z5, z4 * (-F_0_390180644) + z5
    o[7] = _descale(tmp4 + z1 + z3, sh)
    o[5] = _descale(tmp5 + z2 + z4, sh)
    o[3] = _descale(tmp6 + z2 + z3, sh)
    o[1] = _descale(tmp7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """[..., 8, 8] samples minus 128 (row, column) -> [..., 8, 8] coefficients, 8x the true DCT"""
    rows = _fdct_1d(blocks.astype(np.int64), True)
    return np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """[..., 64] by table [64]: d = q << 3, (|c| + d/2) / d with the sign restored"""
    d = q.astype(np.int64) << 3
    mag = (np.abs(coef) + (d >> 1)) // d
    return np.where(coef < 0, -mag, mag)


def geometry(width: int, height: int, subsampling: str) -> dict:
    hs, vs = SAMPLINGS[subsampling]
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    return {"width": width, "height": height, "components": 3, "h_samp": [hs, 1, 1], "v_samp": [vs, 1, 1], "mcus_x": mx, "mcus_y": my}


def forward(rgb: np.ndarray, quality: int = 95, subsampling: str = "4:2:0"):
    """[H, W, 3] u8 RGB -> (info, int16 coefficients in the library's layout, [2, 64] tables)"""
    H, W, _ = rgb.shape
    info = geometry(W, H, subsampling)
    hmax, vmax = info["h_samp"][0], info["v_samp"][0]
    qt = quant_tables(quality)
    out = []
    for c, plane in enumerate(rgb_to_ycc(rgb)):
        hc, vc = info["h_samp"][c], info["v_samp"][c]
        fh, fv = hmax // hc, vmax // vc
        rbx, rby = -(-(-(-W * hc // hmax)) // 8), -(-(-(-H * vc // vmax)) // 8)          # real blocks
        p = _pad_right(plane, rbx * 8 * fh)
        p = _pad_bottom(p, -(-H // fv) * fv)
        if (fh, fv) == (2, 2):
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2
        else:
            assert (fh, fv) == (1, 1)
        p = _pad_bottom(p, rby * 8)[:, :rbx * 8]
        blocks = p.reshape(rby, 8, rbx, 8).transpose(0, 2, 1, 3) - 128
        real = quantise(fdct_islow(blocks).reshape(rby, rbx, 64), qt[min(c, 1)])
        bx, by = info["mcus_x"] * hc, info["mcus_y"] * vc
        grid = np.zeros((by, bx, 64), np.int64)
        grid[:rby, :rbx] = real
        for r in range(rby):                         # dummies right of a real row: the DC of the block to their left
            for x in range(rbx, bx):
                grid[r, x, 0] = grid[r, x - 1, 0]
        for r in range(rby, by):                     # dummy rows: the DC of the last block of the row above in the same MCU
            for x in range(bx):
                grid[r, x, 0] = grid[r - 1, (x // hc) * hc + hc - 1, 0]
        out.append(grid.reshape(-1))
    return info, np.concatenate(out).astype(np.int16), qt


# ----------------------------------------------------------------------------- Annex F scan writer
def _huff_codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    codes, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            codes[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return codes


DC_CODES = [_huff_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
AC_CODES = [_huff_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _block(w, zz, pred, t):
    diff = int(zz[0]) - pred
    s = abs(diff).bit_length()
    w.put(*DC_CODES[t][s])
    if s:
        w.put((diff if diff > 0 else diff - 1) & ((1 << s) - 1), s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*AC_CODES[t][0xF0])
            run -= 16
        s = abs(v).bit_length()
        w.put(*AC_CODES[t][(run << 4) | s])
        w.put((v if v > 0 else v - 1) & ((1 << s) - 1), s)
        run = 0
    if run:
        w.put(*AC_CODES[t][0x00])


def scan_bytes(info: dict, coef: np.ndarray, restart_mcus: int = 0) -> bytes:
    """the entropy-coded segment (between SOS and EOI) of one interleaved scan, restart markers included"""
    mx, my = info["mcus_x"], info["mcus_y"]
    hs, vs = info["h_samp"], info["v_samp"]
    bx = [mx * hs[c] for c in range(3)]
    offs = np.concatenate([[0], np.cumsum([bx[c] * my * vs[c] * 64 for c in range(3)])])
    zz = np.asarray(ZIGZAG)
    w = _BitWriter()
    pred = [0, 0, 0]
    n = 0
    for y in range(my):
        for x in range(mx):
            if restart_mcus and n and n % restart_mcus == 0:
                w.flush()
                w.out += bytes([0xFF, 0xD0 + ((n // restart_mcus - 1) & 7)])
                pred = [0, 0, 0]
            for c in range(3):
                for v in range(vs[c]):
                    for h in range(hs[c]):
                        base = int(offs[c]) + ((y * vs[c] + v) * bx[c] + x * hs[c] + h) * 64
                        blk = coef[base:base + 64][zz]
                        _block(w, blk, pred[c], min(c, 1))
                        pred[c] = int(blk[0])
            n += 1
    w.flush()
    return bytes(w.out)


# ----------------------------------------------------------------------------- files
def split_segments(data: bytes):
    """-> (list of (marker, payload) up to and including SOS, scan bytes without the EOI)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    pos, segs = 2, []
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        ln = (data[pos + 2] << 8) | data[pos + 3]
        segs.append((m, bytes(data[pos + 4:pos + 2 + ln])))
        pos += 2 + ln
        if m == 0xDA:
            return segs, bytes(data[pos:-2])


def segments_of(segs, marker):
    return [p for m, p in segs if m == marker]


def pil_encode(rgb: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0) -> bytes:
    import io

    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart_mcus} if restart_mcus else {}
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling], **kw)
    return buf.getvalue()
