"""Integer model of the snapshot enhancer: Pillow's Image.resize(BICUBIC) and ImageFilter.UnsharpMask on 8-bit images, restated in
numpy (per channel; the channel order does not matter).  The specification the device kernels (csrc/enhance_kernels.hip) and the
host tables (csrc/enhance_api.cpp) are held to; tests/test_enhance_model.py ties it to Pillow itself, byte for byte.

Only the tap weights and the box blur's two weights need floating point: double for the taps and the box radius, float for the
box weight (box_params)."""
import math

import numpy as np

PRECISION_BITS = 22          # Resample.c: 32 - 8 - 2
MAX_TAPS = 5                 # bicubic, support 2, never downscaling


def bicubic(t: float) -> float:
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def taps(n_in: int, n_out: int):
    """-> [(first, [k ...])] per output sample of one axis, n_out >= n_in; weights scaled by 2^22"""
    assert n_out >= n_in >= 1
    scale = n_in / n_out
    support = 2.0
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [bicubic(x + xmin - center + 0.5) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
        assert 1 <= len(k) <= MAX_TAPS
        out.append((xmin, k))
    return out


def _resample_axis(img: np.ndarray, n_out: int, axis: int) -> np.ndarray:
    """one pass along `axis` of a [h, w, c] u8 image; an axis that keeps its size is not touched"""
    n_in = img.shape[axis]
    if n_out == n_in:
        return img
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx, (first, k) in enumerate(taps(n_in, n_out)):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for j, kj in enumerate(k):
            acc += src[first + j] * kj
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resample(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """Image.resize((out_w, out_h), BICUBIC): the horizontal pass over the whole image into an 8-bit image, then the vertical one"""
    return _resample_axis(_resample_axis(img, out_w, 1), out_h, 0)


def box_params(radius: float):
    """BoxBlur.c: the box radius of one of the three passes of a Gaussian of `radius` -> (r, ww, fw)"""
    f32 = np.float32
    rad = float(f32(radius))                     # the radius arrives as a C float; the box radius is computed in double ...
    sigma2 = rad * rad / 3
    L = math.sqrt(12 * sigma2 + 1)
    l = math.floor((L - 1) / 2)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) ** 2))
    fr = f32(l + a)                              # ... and handed on as a float; the weight below is float arithmetic
    r = int(fr)
    ww = int(f32(f32(1 << 24) / f32(fr * f32(2) + f32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _box_axis(img: np.ndarray, r: int, ww: int, fw: int, axis: int) -> np.ndarray:
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    n = src.shape[0]
    idx = np.arange(n)
    acc = np.zeros_like(src)
    for d in range(-r, r + 1):
        acc += src[np.clip(idx + d, 0, n - 1)]
    edge = src[np.clip(idx - r - 1, 0, n - 1)] + src[np.clip(idx + r + 1, 0, n - 1)]
    out = (ww * acc + fw * edge + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(np.moveaxis(out.astype(np.uint8), 0, axis))


def gaussian_blur(img: np.ndarray, radius: float) -> np.ndarray:
    """ImageFilter.GaussianBlur(radius): three box passes along the rows, then three along the columns, each into an 8-bit image"""
    r, ww, fw = box_params(radius)
    out = img
    for axis in (1, 1, 1, 0, 0, 0):
        out = _box_axis(out, r, ww, fw, axis)
    return out


def unsharp_parts(img: np.ndarray, radius: float, percent: int, threshold: int):
    """-> (out, d, unclipped): the result, d = in - blur, and in + d * percent / 100 before the clip (C division: toward zero)"""
    blur = gaussian_blur(img, radius).astype(np.int64)
    src = img.astype(np.int64)
    d = src - blur
    prod = d * int(percent)
    quot = np.where(prod < 0, -((-prod) // 100), prod // 100)
    unclipped = src + quot
    out = np.where(np.abs(d) > int(threshold), np.clip(unclipped, 0, 255), src).astype(np.uint8)
    return out, d, unclipped


def unsharp(img: np.ndarray, radius: float = 1.0, percent: int = 120, threshold: int = 3) -> np.ndarray:
    return unsharp_parts(img, radius, percent, threshold)[0]


def enhance(img: np.ndarray, out_w: int, out_h: int, radius: float = 1.0, percent: int = 120, threshold: int = 3, sharpen: bool = True) -> np.ndarray:
    """[h, w, 3] u8 -> [out_h, out_w, 3] u8: what the device writes for a crop"""
    out = resample(img, out_w, out_h)
    return unsharp(out, radius, percent, threshold) if sharpen else out


def enhanced_size(w: int, h: int, upscale: float = 2.0, max_pixels: int = 4_000_000):
    """the reference's _safe_resize_params (services/enhancer.py:49-62)"""
    new_w = int(round(w * upscale))
    new_h = int(round(h * upscale))
    if new_w * new_h > max_pixels:
        scale = (max_pixels / (w * h)) ** 0.5
        new_w = max(1, int(round(w * scale)))
        new_h = max(1, int(round(h * scale)))
    return new_w, new_h


def pillow_enhance(img: np.ndarray, out_w: int, out_h: int, radius: float = 1.0, percent: int = 120, threshold: int = 3, sharpen: bool = True) -> np.ndarray:
    """the same through Pillow itself, following the reference's rule: resample only when the size grows"""
    from PIL import Image, ImageFilter
    im = Image.fromarray(img)
    if (out_w, out_h) != im.size:
        im = im.resize((out_w, out_h), Image.BICUBIC)
    if sharpen:
        im = im.filter(ImageFilter.UnsharpMask(radius=radius, percent=percent, threshold=threshold))
    return np.asarray(im)
