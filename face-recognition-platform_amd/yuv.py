"""Decoded video surfaces: the frames of cameras that speak H.264 / H.265 (RTSP, most IP cameras), for callers
that bring their own decoder.

The reference reads every source through `cv2.VideoCapture(source)` (backend/app/routes/camera.py:52,185-221), which decodes on
the host and hands out BGR.  No codec ships with this package - but every decoder (a hardware video block, VA-API, ffmpeg in
software) emits the same thing: 8-bit YUV 4:2:0 surfaces with row pitches, NV12 or I420, often already in device memory.
`YuvFrame` holds one such surface (numpy planes, or device addresses and pitches), `YuvBatch` a batch of one geometry, which
`FaceService.process_frames / process_stream` accept in place of a pixel array: `Engine.upload_yuv_async` moves 1.5 bytes per
pixel instead of 3 (or none, for device surfaces) and converts to BGR on the GPU (csrc/yuv_kernels.hip).

The conversion is a contract of exact integers (include/frp.h has it in full): chroma replicated - pixel (x, y) takes the sample
at (x >> 1, y >> 1) -, BT.601 / BT.709 limited range in 20-bit fixed point, or libjpeg's full-range rule ("JFIF").  `to_bgr` is
its numpy form: what `YuvBatch.decode()` gives engines without the device path.  The 601 constants are believed to be OpenCV's;
parity with cv2 is neither claimed nor tested.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

import numpy as np

LAYOUTS = ("NV12", "NV21", "I420", "YV12")
SEMI_PLANAR = ("NV12", "NV21")
# matrix -> yoff, cy, cvr, cvg, cug, cub, rounding, shift:
#   y = max(0, Y - yoff) * cy;  R = (y + cvr v + rnd) >> sh;  G = (y - cvg v - cug u + rnd) >> sh;  B = (y + cub u + rnd) >> sh
# (JFIF: Y + ((c v + 32768) >> 16) is that expression with cy = 65536 - Y << 16 has no bits below the shift)
MATRICES = {"BT601": (16, 1220542, 1673527, 852492, 409993, 2116026, 1 << 19, 20),
            "BT709": (16, 1220542, 1880097, 558891, 223347, 2214593, 1 << 19, 20),
            "JFIF": (0, 65536, 91881, 46802, 22554, 116130, 32768, 16)}


def _check(layout: str, matrix: str) -> None:
    if layout not in LAYOUTS:
        raise ValueError(f"unknown YUV layout {layout!r} (one of {LAYOUTS})")
    if matrix not in MATRICES:
        raise ValueError(f"unknown YUV matrix {matrix!r} (one of {tuple(MATRICES)})")


def split_chroma(c1: np.ndarray, c2: Optional[np.ndarray], layout: str) -> Tuple[np.ndarray, np.ndarray]:
    """the chroma planes in the order the layout names them -> (U, V) [..., H/2, W/2]; semi-planar: c1 is [..., H/2, W] interleaved"""
    if layout in SEMI_PLANAR:
        a, b = c1[..., 0::2], c1[..., 1::2]
        return (a, b) if layout == "NV12" else (b, a)
    return (c1, c2) if layout == "I420" else (c2, c1)


def to_bgr(y: np.ndarray, c1: np.ndarray, c2: Optional[np.ndarray] = None, layout: str = "NV12", matrix: str = "BT601") -> np.ndarray:
    """Y [..., H, W] u8 and the chroma planes in the layout's order (split_chroma) -> BGR [..., H, W, 3] u8, by the contract above.
    Any strides; int32 throughout (every intermediate is below 5.8e8)."""
    _check(layout, matrix)
    y = np.asarray(y)
    H, W = y.shape[-2:]
    if H % 2 or W % 2 or H <= 0 or W <= 0:
        raise ValueError(f"YUV 4:2:0 frames need an even width and height, not {W} x {H}")
    u8, v8 = split_chroma(np.asarray(c1), None if c2 is None else np.asarray(c2), layout)
    if u8.shape[-2:] != (H // 2, W // 2) or v8.shape != u8.shape:
        raise ValueError(f"chroma planes of {u8.shape[-2:]} and {v8.shape[-2:]} under a {H} x {W} Y plane")
    yoff, cy, cvr, cvg, cug, cub, rnd, sh = MATRICES[matrix]
    ytab = (np.maximum(np.arange(256, dtype=np.int32) - yoff, 0) * cy).astype(np.int32)
    yy = ytab[y]
    u = u8.astype(np.int32) - 128
    v = v8.astype(np.int32) - 128

    def up(c):                                     # the term of one chroma sample under its 2 x 2 pixels
        return np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)
    out = np.empty(y.shape + (3,), np.uint8)
    out[..., 0] = np.clip((yy + up(cub * u + rnd)) >> sh, 0, 255)
    out[..., 1] = np.clip((yy + up(-cvg * v - cug * u + rnd)) >> sh, 0, 255)
    out[..., 2] = np.clip((yy + up(cvr * v + rnd)) >> sh, 0, 255)
    return out


class YuvFrame:
    """one decoded surface.  Host: `y` [H, W] u8 and `c1`, `c2` = the chroma planes in the order the layout names them ([H/2, W/2]
    each; semi-planar: `c1` [H/2, W] interleaved, no `c2`) - numpy arrays or views with any row stride: the row pitch is taken from
    the array.  Device: `device=True`, the three are addresses in the engine's GPU, with `hw`, `y_pitch` and `c_pitch` in bytes."""
    __slots__ = ("y", "c1", "c2", "device", "hw", "y_pitch", "c_pitch")

    def __init__(self, y, c1, c2=None, device: bool = False, hw: Optional[Tuple[int, int]] = None,
                 y_pitch: Optional[int] = None, c_pitch: Optional[int] = None):
        self.device = bool(device)
        if self.device:
            if hw is None or y_pitch is None or c_pitch is None:
                raise ValueError("a device surface needs hw, y_pitch and c_pitch")
            self.y, self.c1, self.c2 = int(y), int(c1), (None if c2 is None else int(c2))
            self.hw, self.y_pitch, self.c_pitch = (int(hw[0]), int(hw[1])), int(y_pitch), int(c_pitch)
            return
        self.y, self.c1, self.c2 = (None if a is None else self._plane(a) for a in (y, c1, c2))
        self.hw = tuple(self.y.shape)
        self.y_pitch, self.c_pitch = self.y.strides[0], self.c1.strides[0]
        if self.c2 is not None and (self.c2.shape != self.c1.shape or self.c2.strides[0] != self.c_pitch):
            c = np.ascontiguousarray(self.c1)      # (two chroma planes of unlike pitch: the call takes one c_pitch)
            self.c1, self.c2, self.c_pitch = c, np.ascontiguousarray(self.c2), c.strides[0]

    @staticmethod
    def _plane(a) -> np.ndarray:
        a = np.asarray(a)
        if a.ndim == 3 and a.shape[2] == 2:        # an interleaved plane handed over as [H/2, W/2, 2]
            a = a.reshape(a.shape[0], -1) if a.flags.c_contiguous else np.ascontiguousarray(a).reshape(a.shape[0], -1)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError("a YUV plane is a 2-D uint8 array")
        if a.shape[1] > 1 and a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)            # (column-strided or row-overlapping views: copied once)
        return a

    def packed(self) -> "YuvFrame":
        """a host frame with every plane contiguous"""
        return YuvFrame(np.ascontiguousarray(self.y), np.ascontiguousarray(self.c1), None if self.c2 is None else np.ascontiguousarray(self.c2))


class YuvBatch(list):
    """a batch of decoded surfaces of ONE geometry and layout, all in host memory or all on the device (what FaceService accepts in
    place of a pixel array; mirrors mjpeg.JpegBatch): `hw` = (height, width) of every frame"""

    def __init__(self, frames: Iterable[YuvFrame], layout: str = "NV12", matrix: str = "BT601", hw: Optional[Tuple[int, int]] = None):
        super().__init__(frames)
        self.layout, self.matrix = layout, matrix
        if hw is None:
            if not len(self):
                raise ValueError("an empty YuvBatch needs hw")
            hw = self[0].hw
        self.hw = (int(hw[0]), int(hw[1]))
        self.validate()

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return (len(self), self.hw[0], self.hw[1], 3)

    def validate(self) -> None:
        """raises ValueError for what no path converts: unknown layout / matrix, an odd size, frames of another geometry, planes
        that do not fit the layout, host and device frames mixed"""
        _check(self.layout, self.matrix)
        H, W = self.hw
        if H <= 0 or W <= 0 or H % 2 or W % 2:
            raise ValueError(f"YUV 4:2:0 frames need an even width and height, not {W} x {H}")
        semi = self.layout in SEMI_PLANAR
        for i, f in enumerate(self):
            if f.hw != self.hw:
                raise ValueError(f"frame {i} is {f.hw}, the batch holds {self.hw}")
            if f.device != self[0].device:
                raise ValueError(f"frame {i}: host and device surfaces in one batch")
            if (f.c2 is None) != semi:
                raise ValueError(f"frame {i}: {self.layout} has {'one interleaved chroma plane' if semi else 'two chroma planes'}")
            if not f.device and f.c1.shape != (H // 2, W if semi else W // 2):
                raise ValueError(f"frame {i}: chroma plane of {f.c1.shape} under a {H} x {W} Y plane")

    def plane_table(self):
        """-> (device, y_pitch, c_pitch, [[Y, second, third plane address or 0] per frame], keep-alive): the arguments of
        frp_upload_yuv.  The call takes ONE pitch pair: host frames whose pitches differ are packed first (a copy)."""
        self.validate()
        frames: List[YuvFrame] = list(self)
        if not frames:
            raise ValueError("empty batch")
        if not frames[0].device and any((f.y_pitch, f.c_pitch) != (frames[0].y_pitch, frames[0].c_pitch) for f in frames):
            frames = [f.packed() for f in frames]
        f0 = frames[0]
        if f0.device:
            if any((f.y_pitch, f.c_pitch) != (f0.y_pitch, f0.c_pitch) for f in frames):
                raise ValueError("device surfaces of one batch share their pitches")
            table = [[f.y, f.c1, f.c2 or 0] for f in frames]
        else:
            table = [[f.y.ctypes.data, f.c1.ctypes.data, 0 if f.c2 is None else f.c2.ctypes.data] for f in frames]
        return f0.device, f0.y_pitch, f0.c_pitch, table, frames

    def decode(self) -> np.ndarray:
        """host conversion (to_bgr) -> u8 BGR [B,H,W,3]: the path for engines without the device converter"""
        self.validate()
        out = np.empty(self.shape, np.uint8)
        for i, f in enumerate(self):
            if f.device:
                raise TypeError("device surfaces are converted by the engine (Engine.upload_yuv), not on the host")
            out[i] = to_bgr(f.y, f.c1, f.c2, self.layout, self.matrix)
        return out
