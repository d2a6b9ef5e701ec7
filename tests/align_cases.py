"""The inputs of the alignment tests, shared by the host tests that prove their conditions (tests/test_align_inputs.py) and the GPU
tests that run them (tests/test_gpu_align_exact.py).  Frames are built once, read-only."""
import functools

import numpy as np

from align_model import TEMPLATE32

FLAG_RGB = 2


@functools.lru_cache(maxsize=None)
def noise(H, W, seed=0):
    a = np.random.default_rng(1000 + 7 * H + W + seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def smooth(H, W):
    """channels differ, gradients of 1..3 grey levels per pixel with a few wrap-around edges"""
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([(2 * x + y) % 200, (3 * y + x) % 180, (x + 2 * y) % 220], -1).astype(np.uint8)
    a.setflags(write=False)
    return a


def frame(kind, H, W):
    return noise(H, W) if kind == "noise" else smooth(H, W)


# ---------------------------------------------------------------- exact family: landmarks s * template + (Tx, Ty)
def exact_kps64(s, T):
    return s * TEMPLATE32.astype(np.float64) + np.array(T, np.float64)


# (s, (Tx, Ty), (H, W)): the source point of chip pixel (u, v) is exactly (s u + Tx, s v + Ty)
EXACT_CASES = (
    [(1.0, (0, 0), hw) for hw in ((112, 112), (113, 130), (40, 50))]                       # every tap weight exactly 1
    + [(2.0, T, hw) for T in ((0, 0), (13, 21)) for hw in ((224, 224), (260, 250))]        # integer source coordinates
    + [(0.5, T, hw) for T in ((0, 0), (3, 5)) for hw in ((56, 56), (70, 64), (1, 3))]      # weights 1/2 and 1/4; x0 = W-1; bx_max = 1
)


def exact_id(c):
    s, T, (H, W) = c
    return f"s{s:g}_T{T[0]}_{T[1]}_{H}x{W}"


# ---------------------------------------------------------------- general family
def face_kps(faces, seed, mirror=False):
    """as test_align_parity: the template rotated and scaled about its centre, moved to (cx, cy), plus 1.5 px Gaussian jitter"""
    rng = np.random.default_rng(seed)
    out = []
    for (cx, cy, sc, ang) in faces:
        t = TEMPLATE32.astype(np.float64) - 56.0
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        k = (t @ R.T) * sc + rng.standard_normal((5, 2)) * 1.5
        if mirror:
            k[:, 0] = -k[:, 0]          # x -> -x about the face centre: no proper similarity fits, Umeyama's reflection guard acts
        out.append(k + [cx, cy])
    return np.array(out, dtype=np.float32)


# name -> ((H, W), landmarks [M,5,2] float32)
GENERAL_CASES = {
    "240x320_four_faces": ((240, 320), face_kps([(160, 120, 1.5, 0.1), (60, 50, 0.6, -0.4), (300, 220, 2.0, 0.8), (10, 10, 1.0, 0.0)], 5)),
    "64x2048_x_near_2000": ((64, 2048), face_kps([(1990, 30, 0.9, 2.7)], 6)),
    "1088x1920_far_corner": ((1088, 1920), face_kps([(1850, 1000, 3.0, -1.2)], 7)),
    "33x47_down_and_up": ((33, 47), face_kps([(20, 15, 0.25, 0.5), (20, 15, 4.0, 3.1)], 8)),
    "240x320_mirrored": ((240, 320), face_kps([(160, 120, 1.5, 0.1)], 9, mirror=True)),
}
# (case, frame kind, rgb)
GENERAL_RUNS = [(n, k, rgb) for n in GENERAL_CASES for (k, rgb) in (("noise", False), ("smooth", False), ("noise", True))]


# ---------------------------------------------------------------- the pipeline's launch (Engine.align_resident)
PIPE_B, PIPE_K, PIPE_HW = 3, 4, (97, 131)
PIPE_COUNTS = np.array([2, 0, 3], np.int32)


@functools.lru_cache(maxsize=None)
def pipeline_case():
    """-> frames [3,97,131,3] u8, kps [3,4,5,2] float32, exact [3,4] bool (slot holds an exact-family set)"""
    H, W = PIPE_HW
    frames = np.stack([noise(H, W, seed=11), smooth(H, W), noise(H, W, seed=13)])
    kps = np.stack([face_kps([(60, 45, 0.8, 0.3), (0, 0, 1, 0), (90, 60, 1.2, -0.7), (30, 70, 0.5, 1.9)], 20 + b) for b in range(PIPE_B)])
    exact = np.zeros((PIPE_B, PIPE_K), bool)
    for b, k in ((0, 1), (1, 0), (2, 2)):           # one exact-family set per frame, inside the counted faces where there are any
        kps[b, k] = exact_kps64(1.0, (0, 0)).astype(np.float32)
        exact[b, k] = True
    for a in (frames, kps, exact):
        a.setflags(write=False)
    return frames, kps, exact


def pipeline_slots():
    """(b, k) of the chips the compaction lists, in order"""
    return [(b, k) for b in range(PIPE_B) for k in range(int(PIPE_COUNTS[b]))]


# ---------------------------------------------------------------- landmarks without a transform
def degenerate_sets():
    t = TEMPLATE32.copy()
    one_inf = t.copy()
    one_inf[2, 0] = np.inf
    return {
        "five_identical_points": np.full((5, 2), 77.25, np.float32),
        "all_nan": np.full((5, 2), np.nan, np.float32),
        "one_plus_inf": one_inf,
        "all_1e30": np.full((5, 2), 1e30, np.float32),
        "all_minus_1e30": np.full((5, 2), -1e30, np.float32),
    }
