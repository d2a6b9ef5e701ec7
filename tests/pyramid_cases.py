"""Planted per-scale detections for the cross-scale merge of the detection pyramid (not a test module).

A case is what pyramid_merge_kernel reads and what pyramid.merge_scales reads: per scale the detections of B frames
in the coordinates of that scale's resized image, scale-major arrays with P slots per frame and scale.  CASES is a
fixed list (seeded); tests/test_pyramid_host.py proves with merge_scales itself that the list reaches every branch
the kernel can get wrong, tests/test_gpu_pyramid.py holds the kernel to merge_scales on every case.

Rows from the count on are DEAD: they hold junk (finite, large) that neither side may read.
"""
from typing import Dict, List, Optional

import numpy as np

from frp_amd import pyramid

f32 = np.float32
JUNK = f32(7777.0)


def _empty(S, B, P):
    return dict(boxes=np.full((S, B, P, 4), JUNK, f32), kps=np.full((S, B, P, 5, 2), JUNK, f32),
                scores=np.full((S, B, P), JUNK, f32), counts=np.zeros((S, B), np.int32))


def _case(name, frame_hw, det_hws, arrays, K, nms_iou):
    return dict(name=name, frame_hw=tuple(frame_hw), det_hws=[tuple(hw) for hw in det_hws], K=int(K), nms_iou=float(nms_iou), **arrays)


def _put(a, s, b, rows):
    """rows: [(box4, score)] in detector order; landmarks are planted inside the box"""
    for j, (box, score) in enumerate(rows):
        x1, y1, x2, y2 = [f32(v) for v in box]
        a["boxes"][s, b, j] = (x1, y1, x2, y2)
        fx = np.array([0.3, 0.7, 0.5, 0.35, 0.65], f32)
        fy = np.array([0.35, 0.35, 0.55, 0.75, 0.75], f32)
        a["kps"][s, b, j, :, 0] = x1 + (x2 - x1) * fx
        a["kps"][s, b, j, :, 1] = y1 + (y2 - y1) * fy
        a["scores"][s, b, j] = f32(score)
    a["counts"][s, b] = len(rows)


def planted_case(name, seed, frame_hw, scales, B=3, P=16, K=8, nms_iou=0.4, n_obj=12, empty_scale=None, empty_frame=None):
    """n_obj objects per frame; every scale sees most of them, jittered, with scores quantised to sixteenths (ties within
    and across scales), its rows in detector order (score descending) and cut at P.  empty_scale = (frame, scale): that
    frame has no detection at that scale; empty_frame: none at any."""
    rng = np.random.default_rng(seed)
    H, W = frame_hw
    det_hws = [pyramid.scaled_size(H, W, s) for s in scales]
    a = _empty(len(scales), B, P)
    for b in range(B):
        if b == empty_frame:
            continue
        cx, cy = rng.uniform(40, W - 40, n_obj), rng.uniform(40, H - 40, n_obj)
        half = rng.uniform(10, 30, n_obj)
        for s, (hs, ws) in enumerate(det_hws):
            if (b, s) == empty_scale:
                continue
            rx, ry = W / ws, H / hs
            rows = []
            for o in range(n_obj):
                if rng.random() < 0.2:
                    continue                                   # this scale missed the object
                jx, jy, jw = rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.9, 1.1)
                hw_, hh_ = half[o] * jw, half[o] * jw * 1.3
                box = ((cx[o] + jx - hw_) / rx, (cy[o] + jy - hh_) / ry, (cx[o] + jx + hw_) / rx, (cy[o] + jy + hh_) / ry)
                rows.append((box, round(rng.uniform(0.3, 1.0) * 16) / 16))
            rows.sort(key=lambda r: -r[1])                     # stable: detector order
            _put(a, s, b, rows[:P])
    return _case(name, frame_hw, det_hws, a, K, nms_iou)


def exact_iou_case():
    """360 x 500 at scales (1, .5): the half scale's ratio is exactly 2.  nms_iou = 0.5, K = 4.
    frame 0: scale 1 holds the 9 x 18 box (0, 0, 8, 17), the half scale the integer box (0, 0, 4, 4) -> (0, 0, 8, 8), 9 x 9 under
             the +1 convention and inside the first: IoU = 81 / 162 = 0.5 exactly = nms_iou, NOT above it: both are kept.  A third box,
             far away, has the score 0.0 on a live row and is kept too.
    frame 1: the same pair with the large box one fp32 step shorter (y2 = 17 - 2^-19): IoU = nextafter(0.5, 1): suppressed.
    frame 2: nothing at any scale."""
    a = _empty(2, 3, 4)
    _put(a, 0, 0, [((0, 0, 8, 17), 0.9), ((300, 200, 330, 240), 0.0)])
    _put(a, 1, 0, [((0, 0, 4, 4), 0.8)])
    _put(a, 0, 1, [((0, 0, 8, np.nextafter(f32(17), f32(0))), 0.9)])
    _put(a, 1, 1, [((0, 0, 4, 4), 0.8)])
    return _case("exact_iou", (360, 500), [(360, 500), (180, 250)], a, 4, 0.5)


def single_scale_case():
    """one scale at ratio 1, rows as a detector leaves them (score descending, no overlap): the output is the first K inputs"""
    P, K, n = 16, 8, 12
    a = _empty(1, 2, P)
    for b in range(2):
        rows = [((20 + 110 * (i % 4), 15 + 110 * (i // 4), 20 + 110 * (i % 4) + 60 + i, 15 + 110 * (i // 4) + 80 + b),
                 (16 - i // 2) / 16) for i in range(n - 5 * b)]
        _put(a, 0, b, rows)
    return _case("single_scale", (360, 500), [(360, 500)], a, K, 0.4)


def capacity_case():
    """4 scales x 128 slots, every slot live in frame 0 (512 candidates: every thread and sort slot of the kernel), K = 128"""
    rng = np.random.default_rng(4128)
    H, W = 360, 500
    scales = (1.0, 0.5, 0.25, 0.75)
    det_hws = [pyramid.scaled_size(H, W, s) for s in scales]
    a = _empty(4, 2, 128)
    for b, n in ((0, 128), (1, 20)):
        for s, (hs, ws) in enumerate(det_hws):
            rows = []
            for _ in range(n):
                cx, cy, r = rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(3, 12)
                rows.append((((cx - r) * ws / W, (cy - r) * hs / H, (cx + r) * ws / W, (cy + r) * hs / H), round(rng.uniform(0, 1) * 64) / 64))
            rows.sort(key=lambda r: -r[1])
            _put(a, s, b, rows)
    return _case("capacity_4x128", (H, W), det_hws, a, 128, 0.4)


def _build() -> List[Dict]:
    cases = [planted_case(f"planted_{seed}", seed, (360, 500), (1.0, 0.5, 0.25), empty_scale=(1, seed % 3),
                          empty_frame=2 if seed == 3 else None) for seed in range(8)]
    cases += [planted_case(f"inexact_{seed}", 100 + seed, (359, 501), (1.0, 0.5, 0.25)) for seed in range(2)]
    cases += [exact_iou_case(), single_scale_case(), capacity_case()]
    return cases


CASES = _build()


def per_scale(case, frames: Optional[slice] = None):
    """the case as pyramid.merge_scales' first argument"""
    fr = frames if frames is not None else slice(None)
    return [(hw, dict(boxes=case["boxes"][s, fr], kps=case["kps"][s, fr], scores=case["scores"][s, fr], counts=case["counts"][s, fr]))
            for s, hw in enumerate(case["det_hws"])]


_REF = {}


def reference(case, K: Optional[int] = None):
    """pyramid.merge_scales of the case (computed once per case and K; callers must not write into it)"""
    K = case["K"] if K is None else K
    key = (case["name"], K)
    if key not in _REF:
        _REF[key] = pyramid.merge_scales(per_scale(case), case["frame_hw"], K, case["nms_iou"])
        for arr in _REF[key]:
            arr.setflags(write=False)
    return _REF[key]
