"""Shapes, parameter sets and seeded inputs shared by tests/test_enhance_model.py (CPU: model against Pillow) and
tests/test_gpu_enhance.py (device against model and Pillow)."""
import numpy as np

# name -> (w, h, out_w, out_h)
SIZES = {
    "a_1x1": (1, 1, 2, 2),                  # smallest possible
    "b_3x5": (3, 5, 7, 9),                  # fewer samples than taps: every output is a border case
    "c_x2": (53, 37, 106, 74),              # exact x2
    "d_cap": (160, 90, 222, 125),           # the non-integer ratio the pixel cap produces
    "e_same": (41, 33, 41, 33),             # no resample
    "e_one_axis": (41, 33, 60, 33),         # one axis only
    "e_other_axis": (41, 33, 41, 50),
}
# (radius, percent, threshold, sharpen)
PARAMS = [(1.0, 120, 3, True), (2.0, 150, 3, True), (0.5, 500, 1, True), (0.0, 120, 0, True), (1.0, 120, 3, False)]
DEFAULT = PARAMS[0]


def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[h, w, 3] u8.  "noise": uniform bytes.  "ramp": a smooth field - a tilted plane plus two slow waves with seeded phases - scaled
    to overshoot 0..255 a little and clipped, so it has gentle slopes (differences to the blur around the threshold) and flat
    saturated regions with soft shoulders"""
    rng = np.random.default_rng([seed, h, w, 0 if kind == "noise" else 1])
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    assert kind == "ramp"
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3), np.uint8)
    for c in range(3):
        ph = rng.uniform(0, 2 * np.pi, size=3)
        fx, fy = rng.uniform(0.15, 0.6, size=2)
        v = 128 + 90 * np.sin(fx * xx + ph[0]) + 70 * np.sin(fy * yy + ph[1]) + 40 * np.sin(0.23 * (xx + yy) + ph[2])
        out[..., c] = np.clip(v, 0, 255)
    return out
