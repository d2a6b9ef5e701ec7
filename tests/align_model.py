"""Float64 reference of face alignment (align_kernel, csrc/aux_kernels.hip) with a derived per-pixel error bound, and an fp32
transcription of the kernel's arithmetic for the host tests.

reference()         plain float64: Umeyama similarity of the float32 landmarks against the float32-rounded ArcFace template, inverse
                    map per output pixel, bilinear interpolation of the zero-padded frame, (RGB - 127.5) / 127.5.  The GPU tests compare
                    the device's chips with this and with nothing else.
tol                 per pixel and channel, the sum of three terms, none of them fitted to the kernel:
  1 coordinate      (dx * Gx + dy * Gy) / 127.5.  The kernel keeps the six inverse coefficients and evaluates sx = i00 u + i01 v + i02 in
                    fp32: three coefficient roundings, two products and two sums, each off by at most 2^-24 of a magnitude no larger than
                    B = |Ai00| u + |Ai01| v + |Ai02|, so |sx_fp32 - sx| <= 7 * 2^-24 * B < dx = 2^-21 * B (likewise dy).  The zero-border
                    bilinear interpolant is continuous and piecewise bilinear: moving the source point by d in x changes the value by at
                    most d times the largest horizontal neighbour difference of the cells it passes through.  Gx / Gy are those maxima
                    over pixels x0-1..x0+2, y0-1..y0+2 of the zero-padded frame (the cell and its eight neighbours: dx, dy << 1, so a
                    crossed cell boundary stays inside the window), maximum over channels.
  2 accumulation    4e-6: the fp32 weights (1-ax, 1-ay and four products: relative 3 * 2^-24 each), four multiply-adds and the
                    normalisation (one subtraction, the rounded constant 1/127.5, one product).  The weights sum to 1 and the taps are
                    <= 255, so the value is off by at most 12 * 2^-24 * 255 before and 12 * 2^-24 * 255 / 127.5 + 2 * 2^-24 ~ 1.6e-6 after
                    the normalisation.
  3 fp16 rounding   half an fp16 ulp of |blob| (exponent floor 2^-14: subnormal spacing 2^-24), times 1 + 1e-3 for the ulp of a value
                    that terms 1 and 2 moved.
kernel_fp32_model() the kernel's arithmetic in numpy float32 (double closed form, six fp32 coefficients, fp32 per-pixel map, floor, weights,
                    accumulate, normalise, fp16), with or without fused multiply-adds.  HOST TESTS ONLY: it shows that each GPU input is one
                    where fp32 arithmetic can meet the bound (tests/test_align_inputs.py).  No GPU assertion compares against it.
"""
import numpy as np

from oracle import network as onet

CHIP = 112
TEMPLATE32 = onet.ARCFACE_TEMPLATE.astype(np.float32)          # the kernel's kTemplate: the template rounded to float32
ACC_TERM = 4e-6
_PAD = 4


def similarity(kps_f32):
    """2x3 float64, landmarks -> template: Umeyama on the float32 landmarks and the float32-rounded template, both cast to float64"""
    k = np.asarray(kps_f32, np.float32).reshape(5, 2).astype(np.float64)
    return onet.umeyama_similarity(k, TEMPLATE32.astype(np.float64))


def closed_form(kps_f32):
    """The kernel's closed form of the same least-squares problem over proper similarities [[a,-b],[b,a]] + t, float64.
    -> (2x3 matrix, ok); ok False: degenerate landmarks (the kernel then writes the border value everywhere)"""
    k = np.asarray(kps_f32, np.float32).reshape(5, 2).astype(np.float64)
    t = TEMPLATE32.astype(np.float64)
    with np.errstate(all="ignore"):
        ms, md = k.sum(0) / 5, t.sum(0) / 5
        s, d = k - ms, t - md
        num_a = (s[:, 0] * d[:, 0] + s[:, 1] * d[:, 1]).sum()
        num_b = (s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]).sum()
        den = (s * s).sum()
        ok = bool(den > 1e-12 and (num_a * num_a + num_b * num_b) > 1e-24)
        a, b = (num_a / den, num_b / den) if ok else (1.0, 0.0)
        tx, ty = md[0] - (a * ms[0] - b * ms[1]), md[1] - (b * ms[0] + a * ms[1])
    return np.array([[a, -b, tx], [b, a, ty]]), ok


def _inverse(M):
    return np.linalg.inv(np.vstack([M, [0.0, 0.0, 1.0]]))[:2]


def _rgb(frame_u8, rgb):
    f = np.asarray(frame_u8)
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
    return f if rgb else f[..., ::-1]


def reference(frame_u8, kps_f32, rgb=False):
    """frame [H,W,3] u8 (BGR; RGB with rgb=True), five float32 landmarks -> (blob [112,112,3] float64 RGB, tol [112,112,3] float64)"""
    img = _rgb(frame_u8, rgb).astype(np.float64)
    H, W, _ = img.shape
    Ai = _inverse(similarity(kps_f32))
    v, u = np.meshgrid(np.arange(CHIP, dtype=np.float64), np.arange(CHIP, dtype=np.float64), indexing="ij")
    sx = Ai[0, 0] * u + Ai[0, 1] * v + Ai[0, 2]
    sy = Ai[1, 0] * u + Ai[1, 1] * v + Ai[1, 2]
    # the zero-padded frame: pixel (x, y) at P[y + _PAD, x + _PAD]; a cell further out than the padding reads the same zeros
    P = np.zeros((H + 2 * _PAD, W + 2 * _PAD, 3))
    P[_PAD:_PAD + H, _PAD:_PAD + W] = img
    fx0, fy0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - fx0)[..., None], (sy - fy0)[..., None]
    px = np.clip(fx0, -(_PAD - 1), W + 1).astype(np.int64) + _PAD         # keeps px-1 .. px+2 inside P
    py = np.clip(fy0, -(_PAD - 1), H + 1).astype(np.int64) + _PAD
    top = P[py, px] * (1 - ax) + P[py, px + 1] * ax
    bot = P[py + 1, px] * (1 - ax) + P[py + 1, px + 1] * ax
    blob = ((top * (1 - ay) + bot * ay) - 127.5) / 127.5
    # term 1
    DX = np.abs(P[:, 1:] - P[:, :-1]).max(-1)          # DX[y, x]: between columns x and x+1
    DY = np.abs(P[1:, :] - P[:-1, :]).max(-1)          # DY[y, x]: between rows y and y+1
    Gx = np.zeros((CHIP, CHIP))
    Gy = np.zeros((CHIP, CHIP))
    for j in range(-1, 3):
        for i in range(-1, 2):
            Gx = np.maximum(Gx, DX[py + j, px + i])
            Gy = np.maximum(Gy, DY[py + i, px + j])
    dx = 2.0 ** -21 * (abs(Ai[0, 0]) * u + abs(Ai[0, 1]) * v + abs(Ai[0, 2]))
    dy = 2.0 ** -21 * (abs(Ai[1, 0]) * u + abs(Ai[1, 1]) * v + abs(Ai[1, 2]))
    coord = (dx * Gx + dy * Gy) / 127.5
    # term 3
    e = np.floor(np.log2(np.maximum(np.abs(blob), 2.0 ** -14)))
    half_ulp = 0.5 * 2.0 ** (e - 10)
    tol = coord[..., None] + ACC_TERM + half_ulp * (1 + 1e-3)
    return blob, tol


def within(chips_f16, blob, tol):
    """the GPU assertion's predicate of the general family: |chips - blob| <= tol on every pixel and channel"""
    return bool(np.all(np.abs(np.asarray(chips_f16).astype(np.float64) - blob) <= tol))


def worst(chips_f16, blob, tol):
    """largest err / tol (reported, never asserted on its own)"""
    return float((np.abs(np.asarray(chips_f16).astype(np.float64) - blob) / tol).max())


def _fma(a, b, c, fma):
    """a * b + c on float32 arrays: one rounding (through float64: the product of two float32 is exact there) or two"""
    if fma:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return (a * b).astype(np.float32) + c


def kernel_fp32_model(frame_u8, kps_f32, rgb=False, fma=False, mutant=None):
    """-> [112,112,3] float16 RGB.  mutant (host tests: each must break the GPU predicate): 'swap_ax' exchanges the two horizontal
    weights, 'replicate' treats the border as replicated instead of 0."""
    f32 = np.float32
    img = _rgb(frame_u8, rgb)
    H, W, _ = img.shape
    M, ok = closed_form(kps_f32)
    a, b, tx, ty = M[0, 0], M[1, 0], M[0, 2], M[1, 2]
    with np.errstate(all="ignore"):
        det = a * a + b * b
        i00, i01, i10, i11 = f32(a / det), f32(b / det), f32(-b / det), f32(a / det)
        itx, ity = f32(-(a * tx + b * ty) / det), f32(-(-b * tx + a * ty) / det)
        v, u = np.meshgrid(np.arange(CHIP, dtype=f32), np.arange(CHIP, dtype=f32), indexing="ij")
        sx = _fma(np.full_like(u, i00), u, (i01 * v).astype(f32), fma) + itx
        sy = _fma(np.full_like(u, i10), u, (i11 * v).astype(f32), fma) + ity
        sx = np.fmin(np.fmax(sx, f32(-2)), f32(W + 1)).astype(f32)     # fmaxf / fminf: NaN lands on a bound
        sy = np.fmin(np.fmax(sy, f32(-2)), f32(H + 1)).astype(f32)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    ax, ay = sx - fx0, sy - fy0
    assert ax.dtype == f32 and ay.dtype == f32
    if mutant == "swap_ax":
        ax = f32(1) - ax
    acc = np.zeros((CHIP, CHIP, 3), f32)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            if mutant == "replicate":
                inside = np.ones_like(inside)
            inside &= ok
            w = ((ax if dx else f32(1) - ax) * (ay if dy else f32(1) - ay)).astype(f32)
            w = np.where(inside, w, f32(0))
            tap = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(f32)
            acc = _fma(np.broadcast_to(w[..., None], tap.shape), tap, acc, fma)
    out = ((acc - f32(127.5)) * f32(f32(1.0) / f32(127.5))).astype(f32)
    return out.astype(np.float16)
