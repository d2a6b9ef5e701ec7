"""Reference of the YUV 4:2:0 -> BGR contract (include/frp.h: frp_upload_yuv), written from the formulas and not from the package's
code: a scalar form on Python integers and a vectorised form on int64.  Tests only."""
import functools

import numpy as np

# limited range, 2^20 fixed point: CY, CVR, CVG, CUG, CUB = round(c * 2^20) of the three-decimal coefficients
LIMITED = {"BT601": (1220542, 1673527, 852492, 409993, 2116026),
           "BT709": (1220542, 1880097, 558891, 223347, 2214593)}
assert LIMITED["BT601"] == tuple(round(c * 2 ** 20) for c in (1.164, 1.596, 0.813, 0.391, 2.018))
assert LIMITED["BT709"] == tuple(round(c * 2 ** 20) for c in (1.164, 1.793, 0.533, 0.213, 2.112))
MATRICES = ("BT601", "BT709", "JFIF")
LAYOUTS = ("NV12", "NV21", "I420", "YV12")

# the issue's anchor pixels, computed by hand: (Y, U, V) -> (B, G, R) under 601, 709, JFIF
ANCHORS = [
    ((16, 128, 128), (0, 0, 0), (0, 0, 0), (16, 16, 16)),
    ((235, 128, 128), (255, 255, 255), (255, 255, 255), (235, 235, 235)),
    ((126, 128, 128), (128, 128, 128), (128, 128, 128), (126, 126, 126)),
    ((81, 90, 240), (0, 0, 254), (0, 24, 255), (14, 14, 238)),
    ((145, 54, 34), (1, 255, 0), (0, 216, 0), (14, 238, 13)),
    ((41, 240, 110), (255, 0, 0), (255, 15, 0), (239, 15, 16)),
    ((0, 0, 0), (0, 154, 0), (0, 95, 0), (0, 135, 0)),
    ((255, 255, 255), (255, 125, 255), (255, 183, 255), (255, 121, 255)),
    ((200, 1, 254), (0, 161, 255), (0, 174, 255), (0, 154, 255)),
]


def _clamp(x):
    return 0 if x < 0 else 255 if x > 255 else x


def pixel(Y, U, V, matrix):
    """-> (B, G, R); Python integers, >> floors"""
    Y, U, V = int(Y), int(U), int(V)
    u, v = U - 128, V - 128
    if matrix == "JFIF":
        return (_clamp(Y + ((116130 * u + 32768) >> 16)), _clamp(Y + ((-22554 * u - 46802 * v + 32768) >> 16)),
                _clamp(Y + ((91881 * v + 32768) >> 16)))
    CY, CVR, CVG, CUG, CUB = LIMITED[matrix]
    y = max(0, Y - 16) * CY
    return (_clamp((y + CUB * u + 2 ** 19) >> 20), _clamp((y - CVG * v - CUG * u + 2 ** 19) >> 20), _clamp((y + CVR * v + 2 ** 19) >> 20))


def chroma_uv(c1, c2, layout):
    """the chroma planes as the layout orders them (semi-planar: c1 [..., H/2, W] interleaved, c2 None) -> U, V [..., H/2, W/2]"""
    if layout == "NV12":
        return c1[..., 0::2], c1[..., 1::2]
    if layout == "NV21":
        return c1[..., 1::2], c1[..., 0::2]
    if layout == "I420":
        return c1, c2
    if layout == "YV12":
        return c2, c1
    raise ValueError(layout)


def frames(planes, layout, matrix):
    """planes = (Y [B, H, W], c1, c2 or None) u8 arrays, chroma in the layout's order -> BGR [B, H, W, 3] u8.  Chroma replicated:
    pixel (x, y) takes the sample at (x >> 1, y >> 1)."""
    Y, c1, c2 = planes
    U, V = chroma_uv(np.asarray(c1), None if c2 is None else np.asarray(c2), layout)
    B, H, W = Y.shape
    assert H % 2 == 0 and W % 2 == 0 and U.shape == V.shape == (B, H // 2, W // 2)
    u, v = U.astype(np.int64) - 128, V.astype(np.int64) - 128
    Yl = Y.astype(np.int64)

    def up(c):                                  # sample (x >> 1, y >> 1) under pixel (x, y)
        return np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    out = np.empty((B, H, W, 3), np.uint8)
    if matrix == "JFIF":
        terms = ((116130 * u + 32768) >> 16, (-22554 * u - 46802 * v + 32768) >> 16, (91881 * v + 32768) >> 16)
        for ch, t in enumerate(terms):
            out[..., ch] = np.clip(Yl + up(t), 0, 255)
    else:
        CY, CVR, CVG, CUG, CUB = LIMITED[matrix]
        y = np.maximum(0, Yl - 16) * CY
        terms = (CUB * u + 2 ** 19, -CVG * v - CUG * u + 2 ** 19, CVR * v + 2 ** 19)
        for ch, t in enumerate(terms):
            out[..., ch] = np.clip((y + up(t)) >> 20, 0, 255)
    return out


def all_triples(width=4096, n_frames=4):
    """every (Y, U, V) triple exactly once as NV12 planes: each of the 65,536 chroma pairs sits under 64 luma 2 x 2 blocks that hold
    the 256 luma values.  -> (Y [n, H, W], UV [n, H/2, W]) with n * H * W = 2^24; `width` a multiple of 128 that divides 2^24 / n / 2"""
    blocks_x = width // 2                       # chroma samples per row
    assert width % 128 == 0 and (1 << 22) % (blocks_x * n_frames) == 0
    rows = (1 << 22) // blocks_x // n_frames    # chroma rows per frame
    s = np.arange(1 << 22, dtype=np.int64).reshape(n_frames, rows, blocks_x)     # sample index: pair = s >> 6, luma group = s & 63
    pair, grp = s >> 6, s & 63
    UV = np.empty((n_frames, rows, width), np.uint8)
    UV[..., 0::2] = pair & 255
    UV[..., 1::2] = pair >> 8
    Y = np.empty((n_frames, rows * 2, width), np.uint8)
    for dy in range(2):
        for dx in range(2):
            Y[:, dy::2, dx::2] = grp * 4 + dy * 2 + dx
    return Y, UV


@functools.lru_cache(maxsize=None)
def triples_reference(matrix):
    """frames() of all_triples() for `matrix`, computed once per process and shared read-only"""
    Y, UV = all_triples()
    out = frames((Y, UV, None), "NV12", matrix)
    out.setflags(write=False)
    return out
