"""numpy int64 model of the face-quality sums (tests only): what Engine.face_quality returns for rectangles of u8 frames, written from
FaceService._gray / _laplacian_var - grey = (R*4899 + G*9617 + B*1868 + 8192) >> 14, lap = the 5-point Laplacian of grey with
BORDER_REFLECT_101 at the edges of the crop (np.pad(mode="reflect"), which maps a size-1 axis onto itself)."""
import numpy as np


def sums(frames, rect, rgb=False):
    """frames u8 [B,H,W,3]; rect = (frame, top, right, bottom, left) -> int64 [4]: sum g, sum g^2, sum lap, sum lap^2"""
    f, top, right, bottom, left = (int(v) for v in rect)
    crop = frames[f, top:bottom, left:right].astype(np.int64)
    assert crop.size > 0
    r, b = (crop[..., 0], crop[..., 2]) if rgb else (crop[..., 2], crop[..., 0])
    g = (r * 4899 + crop[..., 1] * 9617 + b * 1868 + 8192) >> 14
    p = np.pad(g, 1, mode="reflect")
    lap = p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * g
    return np.array([g.sum(), (g * g).sum(), lap.sum(), (lap * lap).sum()], dtype=np.int64)


def sums_of(frames, rects, rgb=False):
    return np.stack([sums(frames, r, rgb) for r in rects]) if len(rects) else np.zeros((0, 4), np.int64)
