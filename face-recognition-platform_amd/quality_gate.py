"""The quality gate of a frame pass, as a host model (pure Python / numpy): which faces of a pass are worth embedding, decided by the
reference's assess_face_quality (backend/app/services/face_service.py:251-339) on the pass's own detections.  This is the DEFINITION
of the gate - the specification a device implementation between decode and align has to reproduce bit for bit, and the reference of
its tests; nothing on the device runs it yet.  Operation by operation:

  gate_location     box_to_location with every float32 coordinate clamped to [-2^30, 2^30] ahead of the truncation (a device int32
                    conversion and Python's int() then agree); a non-finite coordinate makes the face INVALID.
  sums              S1, S2, L1, L2 of the crop [top:bottom, left:right] exactly as csrc/quality_kernels.hip defines them; an empty
                    crop has none and takes blur = lighting = 50.0, the reference's except branch for crop.size == 0.
  scores_from_sums  float64, ONE rounding per operation, in the order FaceService._pixel_scores and _quality_result write them.  The
                    variances are (N*S2 - S1*S1) / (N*N): an exact integer numerator (N*L2 passes 2^63 for a 4K crop) and one
                    correctly rounded quotient - Python's int / int.  sqrt is correctly rounded.  Squares are x * x: the service
                    writes ** 2, which goes through libm's pow and may differ in the last bit - the reason this is a function of its
                    own and not _quality_result.
  the gate          a face passes iff it is valid, min(fw, fh) >= min_side and overall >= min_score, on the unrounded values.
  compaction        face_slot lists the passing slots b*K + k, frame-major, over k < clamp(counts[b], 0, K).

Per face eight doubles (SCORE_FIELDS); an invalid face has overall = -1.0 and zeros elsewhere."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SCORE_FIELDS = ("overall", "size_score", "position_score", "aspect_score", "blur_score", "lighting_score", "size_ratio", "off")
COORD_LIMIT = float(2 ** 30)
INVALID_SCORES = (-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def check_gate(min_score, min_side) -> Tuple[float, int]:
    """the gate's two bounds: min_score finite and >= 0, min_side an int >= 0 (ValueError otherwise)"""
    ms = float(min_score)
    if not (math.isfinite(ms) and ms >= 0.0):
        raise ValueError("min_score must be finite and >= 0")
    if int(min_side) != min_side or int(min_side) < 0 or int(min_side) > 2 ** 31 - 1:
        raise ValueError("min_side must be an int >= 0")
    return ms, int(min_side)


def gate_location(box, H: int, W: int) -> Optional[Tuple[int, int, int, int]]:
    """(x1, y1, x2, y2) float32 -> (top, right, bottom, left), or None for a non-finite coordinate"""
    v = [float(np.float32(c)) for c in box]
    if not all(math.isfinite(c) for c in v):
        return None
    x1, y1, x2, y2 = (int(min(max(c, -COORD_LIMIT), COORD_LIMIT)) for c in v)
    return max(y1, 0), min(x2, W), min(y2, H), max(x1, 0)


def is_empty(loc) -> bool:
    top, right, bottom, left = loc
    return bottom <= top or right <= left


def variance(n: int, s1: int, s2: int) -> float:
    """(n*s2 - s1*s1) / (n*n) in Python integers: one correctly rounded quotient"""
    return (n * s2 - s1 * s1) / (n * n)


def pixel_scores(n: int, sums) -> Tuple[float, float]:
    """(blur_score, lighting_score) of a crop of n pixels with sums S1, S2, L1, L2 (_pixel_scores on the integer variances)"""
    s1, s2, l1, l2 = (int(v) for v in sums)
    lap_var = variance(n, l1, l2)
    mean = s1 / n
    std = math.sqrt(variance(n, s1, s2))
    blur_score = min(100.0, (lap_var / 500.0) * 100.0)
    brightness = 100.0 - abs(mean - 128.0) / 128.0 * 100.0
    contrast = min(100.0, (std / 50.0) * 100.0)
    return blur_score, (brightness + contrast) / 2.0


def scores_from_sums(H: int, W: int, loc, sums=None) -> Tuple[float, ...]:
    """the eight doubles of a valid face at `loc` in a frame of H x W; sums: S1, S2, L1, L2 of the crop, None for an empty one"""
    top, right, bottom, left = loc
    if is_empty(loc) or sums is None:
        blur_score = lighting_score = 50.0
    else:
        blur_score, lighting_score = pixel_scores((bottom - top) * (right - left), sums)
    fw, fh = max(1, right - left), max(1, bottom - top)
    size_ratio = float(fw * fh) / float(W * H)
    size_score = min(100.0, (size_ratio / 0.25) * 100.0)
    cx, cy = (left + right) / 2.0, (top + bottom) / 2.0
    dx, dy = (cx - W / 2.0) / W, (cy - H / 2.0) / H
    off = math.sqrt(dx * dx + dy * dy)
    position_score = max(0.0, (1.0 - off) * 100.0)
    aspect_score = (min(fw, fh) / max(fw, fh)) * 100.0
    overall = size_score * 0.25 + position_score * 0.2 + aspect_score * 0.2 + blur_score * 0.2 + lighting_score * 0.15
    return overall, size_score, position_score, aspect_score, blur_score, lighting_score, size_ratio, off


def face_passes(loc, scores, min_score: float, min_side: int) -> bool:
    if loc is None:
        return False
    top, right, bottom, left = loc
    return min(max(1, right - left), max(1, bottom - top)) >= min_side and scores[0] >= min_score


def issues_of(loc, scores) -> List[str]:
    """the issue list of _quality_result from the unrounded values of a valid face"""
    top, right, bottom, left = loc
    fw, fh = max(1, right - left), max(1, bottom - top)
    size_ratio, off, blur_score, lighting_score = scores[6], scores[7], scores[4], scores[5]
    issues: List[str] = []
    if size_ratio < 0.05:
        issues.append("Face too small - move closer or crop image")
    if size_ratio > 0.8:
        issues.append("Face too large - image should show some background")
    if off > 0.4:
        issues.append("Face not centered - adjust framing")
    if min(fw, fh) / max(fw, fh) < 0.75:
        issues.append("Face appears distorted or at extreme angle")
    if blur_score < 40:
        issues.append("Image is blurry - use better focus or steady camera")
    if lighting_score < 40:
        issues.append("Poor lighting - improve lighting conditions")
    return issues


def quality_dict(loc, scores) -> Dict:
    """the reference's seven-key dict from the eight doubles of a valid face"""
    s = [float(v) for v in scores]
    return {"score": round(s[0], 2), "size_score": round(s[1], 2), "position_score": round(s[2], 2), "aspect_score": round(s[3], 2),
            "blur_score": round(s[4], 2), "lighting_score": round(s[5], 2), "issues": issues_of(loc, s)}


def crop_sums(frames: np.ndarray, f: int, loc, rgb: bool = False) -> np.ndarray:
    """S1, S2, L1, L2 of the crop as csrc/quality_kernels.hip defines them (numpy int64; the tests have the same in quality_model)"""
    top, right, bottom, left = loc
    crop = frames[f, top:bottom, left:right].astype(np.int64)
    r, b = (crop[..., 0], crop[..., 2]) if rgb else (crop[..., 2], crop[..., 0])
    g = (r * 4899 + crop[..., 1] * 9617 + b * 1868 + 8192) >> 14
    p = np.pad(g, 1, mode="reflect")
    lap = p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * g
    return np.array([g.sum(), (g * g).sum(), lap.sum(), (lap * lap).sum()], dtype=np.int64)


def gate(frames: np.ndarray, boxes, counts: Sequence[int], min_score: float = 0.0, min_side: int = 0, rgb: bool = False,
         sums_of=crop_sums) -> Dict[str, np.ndarray]:
    """The gate of one pass: frames u8 [B,H,W,3], boxes [B,K,4] float32, counts [B] -> scores float64 [B,K,8], passed int32 [B,K],
    rects int32 [B,K,4] (top, right, bottom, left), sums int64 [B,K,4], face_slot int32 [B*K] (-1 behind n_embed), n_embed.  Slots
    at or beyond clamp(counts[b], 0, K) are zero."""
    min_score, min_side = check_gate(min_score, min_side)
    boxes = np.asarray(boxes, np.float32)
    B, K = boxes.shape[:2]
    H, W = frames.shape[1:3]
    out = dict(scores=np.zeros((B, K, 8), np.float64), passed=np.zeros((B, K), np.int32), rects=np.zeros((B, K, 4), np.int32),
               sums=np.zeros((B, K, 4), np.int64), face_slot=np.full((B * K,), -1, np.int32), n_embed=0)
    n = 0
    for b in range(B):
        for k in range(min(max(int(counts[b]), 0), K)):
            loc = gate_location(boxes[b, k], H, W)
            if loc is None:
                out["scores"][b, k] = INVALID_SCORES
                continue
            out["rects"][b, k] = loc
            sums = None
            if not is_empty(loc):
                sums = out["sums"][b, k] = sums_of(frames, b, loc, rgb)
            sc = out["scores"][b, k] = scores_from_sums(H, W, loc, sums)
            if face_passes(loc, sc, min_score, min_side):
                out["passed"][b, k] = 1
                out["face_slot"][n] = b * K + k
                n += 1
    out["n_embed"] = n
    return out
