"""CPU model of the JPEG encoder's OPTIMISED Huffman coding (TEST INFRASTRUCTURE, like tests/jpeg_encode_model.py, whose forward half
and bit writer it imports: imported by tests/ only; the product path is csrc/jpeg_encode_kernels.hip: jpeg_enc_hist_kernel +
csrc/jpeg_encode_api.cpp: optimal_table).

What libjpeg does with optimize_coding (Pillow's save(optimize=True)), restated from the published definitions: a first pass counts the
symbols the scan will code (jchuff.c's gather pass: the DC difference's category per block - predictions reset at restart intervals -
and per non-zero AC coefficient run / size, ZRL per 16 zeros, EOB when the block ends in zeros), jpeg_gen_optimal_table turns every
count table into BITS / HUFFVAL (T.81 K.2 with libjpeg's conventions: a pseudo-symbol 256 of count 1, ties to the larger symbol,
Figure K.3 to limit the lengths to 16), and the scan is coded with those tables, which the four DHT segments carry.
PINNED: tests/test_jpeg_optimize_model.py holds whole files to Pillow's, byte for byte.

Histogram layout = frp_encode_jpeg_histograms': uint32 [544] = dc [2][16] by magnitude category, then ac [2][256] by run / size symbol;
table 0 is Y's, table 1 counts Cb and Cr together.
"""
from __future__ import annotations

import io

import numpy as np

import jpeg_encode_model as M

HIST_ELEMS = 544
AC0 = 32            # first AC bin: ac[t][sym] = hist[AC0 + 256 * t + sym], dc[t][cat] = hist[16 * t + cat]


def _scan_order(info):
    """yields (mcu index, component, first coefficient of the block) in the order of the interleaved scan"""
    mx, my = info["mcus_x"], info["mcus_y"]
    hs, vs = info["h_samp"], info["v_samp"]
    bx = [mx * hs[c] for c in range(3)]
    offs = np.concatenate([[0], np.cumsum([bx[c] * my * vs[c] * 64 for c in range(3)])])
    for y in range(my):
        for x in range(mx):
            for c in range(3):
                for v in range(vs[c]):
                    for h in range(hs[c]):
                        yield y * mx + x, c, int(offs[c]) + ((y * vs[c] + v) * bx[c] + x * hs[c] + h) * 64


def _block_symbols(zz, pred):
    """-> (DC category, DC difference, [(ZRL count, symbol, value)] per non-zero AC, ends in zeros) of one block in zig-zag order"""
    diff = int(zz[0]) - pred
    acs, prev = [], 0
    for k in np.flatnonzero(zz[1:]) + 1:
        k = int(k)
        run, v = k - prev - 1, int(zz[k])
        acs.append((run >> 4, ((run & 15) << 4) | abs(v).bit_length(), v))
        prev = k
    return abs(diff).bit_length(), diff, acs, prev != 63


def histogram(info: dict, coef: np.ndarray, restart_mcus: int = 0) -> np.ndarray:
    """the symbol counts of the scan of `coef` (tests/jpeg_encode_model.forward's layout) -> uint32 [544]"""
    hist = np.zeros(HIST_ELEMS, np.int64)
    zz = np.asarray(M.ZIGZAG)
    pred, last = [0, 0, 0], -1
    for n, c, base in _scan_order(info):
        if restart_mcus and n != last and n and n % restart_mcus == 0:
            pred = [0, 0, 0]
        last = n
        blk = coef[base:base + 64][zz]
        t = min(c, 1)
        cat, _, acs, eob = _block_symbols(blk, pred[c])
        pred[c] = int(blk[0])
        hist[16 * t + cat] += 1
        for zrl, sym, _ in acs:
            hist[AC0 + 256 * t + 0xF0] += zrl
            hist[AC0 + 256 * t + sym] += 1
        if eob:
            hist[AC0 + 256 * t] += 1
    return hist.astype(np.uint32)


def code_sizes(freq):
    """the first half of jpeg_gen_optimal_table: counts [256] -> the code length of every symbol and of the pseudo-symbol [257] BEFORE
    the lengths are limited to 16 (0: the symbol does not occur)"""
    freq = [int(f) for f in freq] + [1]                      # the pseudo-symbol 256: no real symbol gets the all-ones code
    assert len(freq) == 257
    if not any(freq[:256]):
        raise ValueError("all counts are zero")
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):                                 # least frequent; ties: the larger index
            if freq[i] and (v is None or freq[i] <= v):
                c1, v = i, freq[i]
        c2, v = -1, None
        for i in range(257):                                 # the next one
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                c2, v = i, freq[i]
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def gen_optimal_table(freq):
    """jpeg_gen_optimal_table: counts [256] -> (bits [16], vals).  ValueError for counts that are all zero or a code deeper than 32 bits
    (libjpeg: JERR_HUFF_CLEN_OVERFLOW)."""
    codesize = code_sizes(freq)
    if max(codesize) > 32:
        raise ValueError("code deeper than 32 bits")
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):                              # Figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                             # the pseudo-symbol leaves
    vals = [j for ln in range(1, 33) for j in range(256) if codesize[j] == ln]
    return bits[1:17], vals


def tables(hist: np.ndarray):
    """-> [(bits, vals)] x 4 in the order of the DHT segments: DC0, AC0, DC1, AC1"""
    out = []
    for t in (0, 1):
        dc = np.zeros(256, np.int64)
        dc[:16] = hist[16 * t:16 * t + 16]
        out += [gen_optimal_table(dc), gen_optimal_table(hist[AC0 + 256 * t:AC0 + 256 * t + 256])]
    return out


def scan_bytes(info: dict, coef: np.ndarray, restart_mcus: int, tabs) -> bytes:
    """the entropy-coded segment with the codes of `tabs` (as tables() returns them), restart markers included"""
    dc = [M._huff_codes(*tabs[0]), M._huff_codes(*tabs[2])]
    ac = [M._huff_codes(*tabs[1]), M._huff_codes(*tabs[3])]
    zz = np.asarray(M.ZIGZAG)
    w = M._BitWriter()
    pred, last = [0, 0, 0], -1
    for n, c, base in _scan_order(info):
        if restart_mcus and n != last and n and n % restart_mcus == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + ((n // restart_mcus - 1) & 7)])
            pred = [0, 0, 0]
        last = n
        blk = coef[base:base + 64][zz]
        t = min(c, 1)
        cat, diff, acs, eob = _block_symbols(blk, pred[c])
        pred[c] = int(blk[0])
        w.put(*dc[t][cat])
        if cat:
            w.put((diff if diff > 0 else diff - 1) & ((1 << cat) - 1), cat)
        for zrl, sym, v in acs:
            for _ in range(zrl):
                w.put(*ac[t][0xF0])
            w.put(*ac[t][sym])
            s = sym & 15
            w.put((v if v > 0 else v - 1) & ((1 << s) - 1), s)
        if eob:
            w.put(*ac[t][0x00])
    w.flush()
    return bytes(w.out)


def _seg(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def headers(width: int, height: int, quality: int, subsampling: str, restart_mcus: int, tabs) -> bytes:
    """SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1 (`tabs`), DRI (restart_mcus > 0), SOS - Pillow's order"""
    hs, vs = M.SAMPLINGS[subsampling]
    qt = M.quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in (0, 1):
        out += _seg(0xDB, bytes([t]) + bytes(int(qt[t][z]) for z in M.ZIGZAG))
    out += _seg(0xC0, bytes([8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for k, (bits, vals) in enumerate(tabs):
        out += _seg(0xC4, bytes([((k & 1) << 4) | (k >> 1)] + list(bits) + list(vals)))
    if restart_mcus:
        out += _seg(0xDD, bytes([restart_mcus >> 8, restart_mcus & 255]))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0) -> bytes:
    """[H, W, 3] u8 RGB -> the whole file libjpeg writes with optimize_coding"""
    info, coef, _ = M.forward(rgb, quality, subsampling)
    tabs = tables(histogram(info, coef, restart_mcus))
    return headers(rgb.shape[1], rgb.shape[0], quality, subsampling, restart_mcus, tabs) + scan_bytes(info, coef, restart_mcus, tabs) + b"\xff\xd9"


def pil_encode(rgb: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0, optimize: bool = True) -> bytes:
    """Pillow's file.  With optimize its output buffer is max(65536, w * h) bytes (2 * w * h at quality >= 95) and libjpeg cannot
    suspend: an input whose file is larger fails with "Suspension not allowed here" - the callers choose inputs that stay below."""
    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart_mcus} if restart_mcus else {}
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=M.PIL_SUBSAMPLING[subsampling], optimize=optimize, **kw)
    return buf.getvalue()


# ----------------------------------------------------------------------------- the shared cases
def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _smooth(seed, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    base = np.stack([(2 * xx + yy) % 256, (3 * yy + 40) % 256, (xx + 2 * yy + 90) % 256], -1)
    return np.clip(base + rng.integers(-2, 3, size=(h, w, 3)), 0, 255).astype(np.uint8)


def _mixed(seed, h, w):
    """flat 16 x 16 patches + mild noise, a band of strong noise and a smooth ramp: short and long codes in one image"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 255, size=(-(-h // 16), -(-w // 16), 3)).astype(np.float32)
    img = np.repeat(np.repeat(base, 16, axis=0), 16, axis=1)[:h, :w] + rng.normal(0, 6, size=(h, w, 3))
    img[h // 3:h // 3 + h // 8] = rng.integers(0, 256, size=(h // 8, w, 3))
    img[:, :w // 5] = (np.arange(h)[:, None, None] * 255.0 / h)
    return np.clip(img, 0, 255).astype(np.uint8)


def cases():
    """name -> (rgb [H, W, 3], quality, subsampling, restart_mcus); sizes are width x height"""
    flat = np.empty((16, 16, 3), np.uint8)
    flat[:] = (70, 130, 200)
    grey = np.repeat(_noise(6, 48, 48)[..., :1], 3, axis=2)
    return {
        "noise_37x53_q85_420": (_noise(1, 53, 37), 85, "4:2:0", 0),
        "smooth_64x48_q95_444": (_smooth(2, 48, 64), 95, "4:4:4", 0),
        "flat_16x16_q85_420": (flat, 85, "4:2:0", 0),
        "noise_40x72_q20_420_r3": (_noise(4, 72, 40), 20, "4:2:0", 3),
        "noise_33x17_q100_444": (_noise(5, 17, 33), 100, "4:4:4", 0),
        "grey_48x48_q85_420": (grey, 85, "4:2:0", 0),
        "mixed_200x152_q75_420": (_mixed(7, 152, 200), 75, "4:2:0", 0),
        "mixed_320x240_q90_444": (_mixed(8, 240, 320), 90, "4:4:4", 0),
        "mixed_640x480_q85_420": (_mixed(9, 480, 640), 85, "4:2:0", 0),
    }
