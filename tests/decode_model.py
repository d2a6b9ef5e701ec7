"""An integer restatement of decode_nms_kernel's candidate selection, with one switch per plausible kernel error (not a test module).

The selection is restated here on its own: the 36-bit key
    (sortable fp16 logit bits << 20) | (0xFFFFF - anchor index)
with logits that compare equal keyed equally (the two signed zeros included, NaN below -inf), the candidate test, the cap at 1024
and, above the cap, the cut key with its three 12-bit digits - the digits the kernel's radix select walks.  Behind the selection
run the oracle's own box, landmark and score arithmetic: the selected anchors are handed to oracle.network.decode_nms as head maps
whose logits make it take them in the given order without suppressing any, so no box formula is restated here.  The greedy NMS
loop IS restated (float32, one rounding per operation, the +1 areas), because six of the mutants live in it; without a mutant the
whole model must equal decode_cases.reference on every case, which tests/test_decode_inputs.py asserts.

decode(case, mutant=NAME) is the output of a kernel with that one error; test_decode_inputs.py shows that the case list rejects
every one of them under the GPU test's own predicate.
"""
from typing import Dict, Optional

import numpy as np

from oracle import network as onet

f32 = np.float32
CAP = onet.PRE_NMS_CAP
STRIDES = onet.STRIDES

MUTANTS = (
    "ties_to_higher_index",        # key's low bits hold the index itself
    "signed_zeros_split",          # +0.0 keyed above -0.0 (the kernel before this list existed)
    "cap_keeps_lowest",            # above the cap the 1024 LOWEST keys survive
    "cut_one_high",                # the cut key one candidate too high: 1023 survive
    "cut_one_low",                 # ... one too low: 1025 pass, the gather drops the last it meets
    "pass1_ignores_prefix",        # the select's second histogram counts every candidate
    "pass2_ignores_prefix",        # the third one does
    "nms_ge",                      # suppress at IoU >= bound
    "nms_not_greedy",              # suppressed boxes still suppress
    "nms_first_keeper_only",       # only the first kept box suppresses
    "nms_loop_one_short",          # the loop ends one candidate early
    "k_one_short",                 # K - 1 faces at the most
    "xy_swapped",                  # a location's x and y exchanged
    "wl_of_level_0",               # every level's row length taken from level 0
    "level_boundary_one_early",    # the level boundaries one anchor early
    "slot_stride_16",              # the second anchor slot read at channel 16
    "nan_is_candidate",            # threshold mode lets NaN logits pass
    "frame_offset_ignored",        # every frame selects on frame 0's dense logits
)


def sortable16(bits, split_zeros: bool = False):
    """fp16 bit patterns -> 16-bit integers in the order of the values: non-negative 0x8000 + magnitude, negative 0x8000 - magnitude
    (so -0.0 as +0.0), NaN 0 (below -inf = 0x0400).  split_zeros: negative 0x7FFF - magnitude, the complement of the bits, which
    puts -0.0 one below +0.0"""
    h = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    mag = h & 0x7FFF
    out = np.where(h & 0x8000, (0x7FFF if split_zeros else 0x8000) - mag, 0x8000 + mag)
    return np.where(mag > 0x7C00, 0, out)


def keys_of(logits16, idx, mutant: Optional[str] = None):
    """the 36-bit keys of the anchors `idx` with the fp16 logits `logits16`"""
    s = sortable16(np.asarray(logits16, np.float16).view(np.uint16), split_zeros=(mutant == "signed_zeros_split"))
    idx = np.asarray(idx, dtype=np.int64)
    low = idx if mutant == "ties_to_higher_index" else 0xFFFFF - idx
    return (s << 20) | low


def candidates(logits16, lt, mutant: Optional[str] = None):
    """anchor indices that pass the candidate test: logit >= lt as float32; lt == -inf: every anchor, NaN logits included"""
    lg = np.asarray(logits16, np.float16).astype(f32)
    if np.isneginf(lt):
        return np.arange(len(lg))
    with np.errstate(invalid="ignore"):
        ok = ~(lg < f32(lt)) if mutant == "nan_is_candidate" else lg >= f32(lt)
    return np.nonzero(ok)[0]


def digits_of(key: int):
    return (int(key) >> 24) & 0xFFF, (int(key) >> 12) & 0xFFF, int(key) & 0xFFF


def cut_key(logits16, lt) -> Optional[int]:
    """the 1024th largest key of more than 1024 candidates (keys >= it survive), None at or under the cap"""
    cand = candidates(logits16, lt)
    if len(cand) <= CAP:
        return None
    k = np.sort(keys_of(np.asarray(logits16)[cand], cand))[::-1]
    return int(k[CAP - 1])


def radix_select(keys, ignore_prefix_in=()):
    """the kernel's three passes, literally: per pass a 4096-bin histogram of the keys that share the prefix found so far, the digit
    d with count(> d) < need <= count(>= d).  A pass in `ignore_prefix_in` counts every key.  A pass that finds no digit keeps
    the one before (what the kernel's shared variables would still hold)."""
    prefix, need, digit = 0, CAP, 0
    for p in range(3):
        shift = 24 - 12 * p
        sel = keys if (p == 0 or p in ignore_prefix_in) else keys[(keys >> (shift + 12)) == prefix]
        hist = np.bincount((sel >> shift) & 0xFFF, minlength=4096)
        ge = np.cumsum(hist[::-1])[::-1]                 # count(>= d)
        gt = ge - hist
        hit = np.nonzero((gt < need) & (need <= ge))[0]
        if len(hit):
            digit, need = int(hit[0]), need - int(gt[hit[0]])
        prefix = (prefix << 12) | digit
    return prefix


def select(logits16, lt, mutant: Optional[str] = None):
    """anchor indices in the order the NMS sees them: key descending, at most 1024"""
    cand = candidates(logits16, lt, mutant)
    k = keys_of(np.asarray(logits16)[cand], cand, mutant)
    if len(cand) > CAP:
        srt = np.sort(k)[::-1]
        if mutant == "cap_keeps_lowest":
            T, hi = 0, int(srt[-CAP])
            keep = k <= hi
        else:
            if mutant == "cut_one_high":
                T = int(srt[CAP - 2])
            elif mutant == "cut_one_low":
                T = int(srt[CAP])
            elif mutant in ("pass1_ignores_prefix", "pass2_ignores_prefix"):
                T = radix_select(k, ignore_prefix_in=(1,) if mutant == "pass1_ignores_prefix" else (2,))
            else:
                T = int(srt[CAP - 1])
            keep = k >= T
        keep = np.nonzero(keep)[0][:CAP]                 # more than 1024 past the cut: the gather keeps the first it meets
        cand, k = cand[keep], k[keep]
    return cand[np.argsort(-k, kind="stable")]


# ------------------------------------------------------------------------------------------------- geometry
def _levels(canvas_hw):
    return [(canvas_hw[0] // s, canvas_hw[1] // s) for s in STRIDES]


def anchor_table(canvas_hw, mutant: Optional[str] = None):
    """per anchor index: level, the position within the level whose row is read, anchor slot, and the x, y the centre is made of.
    A position past a level's end (level_boundary_one_early) reads the level's first row: whatever the kernel would read there
    is wrong, the model only has to read something defined; x and y come from the position as it is."""
    dims = _levels(canvas_hw)
    n = [2 * h * w for h, w in dims]
    A = sum(n)
    e0, e1 = n[0], n[0] + n[1]
    if mutant == "level_boundary_one_early":
        e0, e1 = e0 - 1, e1 - 1
    idx = np.arange(A)
    level = np.where(idx < e0, 0, np.where(idx < e1, 1, 2))
    li = idx - np.where(level == 0, 0, np.where(level == 1, e0, e1))
    pos, a = li >> 1, li & 1
    wl = np.array([dims[0][1] if mutant == "wl_of_level_0" else w for _, w in dims])[level]
    y = pos // wl
    x = pos - y * wl
    if mutant == "xy_swapped":
        x, y = y, x
    return level, pos % np.array([h * w for h, w in dims])[level], a, x, y


def anchor_values(heads, b, canvas_hw, mutant: Optional[str] = None):
    """[A, 15] fp16: the 15 values the kernel reads for every anchor of frame b"""
    level, pos, a, _, _ = anchor_table(canvas_hw, mutant)
    off = a * (16 if mutant == "slot_stride_16" else 15)
    out = np.zeros((len(level), 15), np.float16)
    for l in range(3):
        rows = np.asarray(heads[l][b]).reshape(-1, 32)
        m = level == l
        out[m] = rows[pos[m][:, None], off[m][:, None] + np.arange(15)[None, :]]
    return out


_BOX_CACHE: Dict = {}


def oracle_boxes(entries):
    """entries: [(level, y, x, a, vals15)] -> (boxes [n, 4], kps [n, 5, 2]) by oracle.network.decode_nms: head maps that hold the
    entries' values with logits n, n-1, ... 1 (every other anchor below the threshold), no suppression (bound 2), K = cap = n"""
    n = len(entries)
    if n == 0:
        return np.zeros((0, 4), f32), np.zeros((0, 5, 2), f32)
    shape = [[1, 1], [1, 1], [1, 1]]
    for l, y, x, a, _ in entries:
        shape[l][0], shape[l][1] = max(shape[l][0], y + 1), max(shape[l][1], x + 1)
    maps = [np.zeros((h, w, 30), f32) for h, w in shape]
    for m in maps:
        m[..., 0] = m[..., 15] = -1.0
    seen = set()
    for i, (l, y, x, a, v) in enumerate(entries):
        assert (l, y, x, a) not in seen
        seen.add((l, y, x, a))
        maps[l][y, x, a * 15:(a + 1) * 15] = np.asarray(v, np.float16).astype(f32)
        maps[l][y, x, a * 15] = n - i
    with np.errstate(invalid="ignore", over="ignore"):
        boxes, kps, _, _ = onet.decode_nms(maps, 0.5, 2.0, n, cap=n)
    assert len(boxes) == n
    return boxes, kps


def _boxes_for(cache_key, order, table, vals, chunk=128):
    """the oracle's boxes and landmarks of the anchors `order`; one oracle call per `chunk` anchors not seen before"""
    store = _BOX_CACHE.setdefault(cache_key, {})
    level, _, a, x, y = table
    todo = [int(i) for i in order if int(i) not in store]
    for c in range(0, len(todo), chunk):
        part = todo[c:c + chunk]
        bx, kp = oracle_boxes([(int(level[i]), int(y[i]), int(x[i]), int(a[i]), vals[i]) for i in part])
        for j, i in enumerate(part):
            store[i] = (bx[j], kp[j])
    n = len(order)
    boxes, kps = np.zeros((n, 4), f32), np.zeros((n, 5, 2), f32)
    for j, i in enumerate(order):
        boxes[j], kps[j] = store[int(i)]
    return boxes, kps


# ------------------------------------------------------------------------------------------------- NMS
def greedy_nms(boxes, K, iou, mutant: Optional[str] = None):
    """positions of the kept boxes: float32, one rounding per operation, a = the kept box, b = the candidate"""
    n = len(boxes) - (1 if mutant == "nms_loop_one_short" else 0)
    K = K - 1 if mutant == "k_one_short" else K
    if n <= 0 or K <= 0:
        return []
    x1, y1, x2, y2 = (boxes[:n, i] for i in range(4))
    one, iou = f32(1), f32(iou)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        area = (x2 - x1 + one) * (y2 - y1 + one)
        supp = np.zeros(n, bool)
        keep = []
        for i in range(n):
            if supp[i]:
                if mutant != "nms_not_greedy":
                    continue
            else:
                keep.append(i)
                if len(keep) >= K:
                    break
                if mutant == "nms_first_keeper_only" and len(keep) > 1:
                    continue
            w = np.maximum(f32(0), np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]) + one)
            h = np.maximum(f32(0), np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]) + one)
            inter = w * h
            ovr = inter / ((area[i] + area[i + 1:]) - inter)
            supp[i + 1:] |= (ovr >= iou) if mutant == "nms_ge" else (ovr > iou)
    return keep


def iou(a, b) -> f32:
    """the NMS's IoU of two boxes (a the kept one), for the case list's own statements"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    one = f32(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        aa, ab = (a[2] - a[0] + one) * (a[3] - a[1] + one), (b[2] - b[0] + one) * (b[3] - b[1] + one)
        w = np.maximum(f32(0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]) + one)
        h = np.maximum(f32(0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]) + one)
        return f32(w * h) / f32(f32(aa + ab) - f32(w * h))


# ------------------------------------------------------------------------------------------------- the whole decode
def thresholds(case):
    """(logit threshold, NMS bound) as the library derives them: forced top-K has no threshold and no suppression"""
    if case["forced"]:
        return f32(-np.inf), f32(2.0)
    return onet.logit_threshold(float(case["det_thresh"])), f32(case["nms_iou"])


def decode_frame(case, b, mutant: Optional[str] = None, K: Optional[int] = None, detail: bool = False):
    K = case["K"] if K is None else K
    lt, bound = thresholds(case)
    geo = mutant if mutant in ("xy_swapped", "wl_of_level_0", "level_boundary_one_early", "slot_stride_16") else None
    table = anchor_table(case["canvas_hw"], geo)
    vals = anchor_values(case["heads"], b, case["canvas_hw"], geo)
    sel_vals = anchor_values(case["heads"], 0, case["canvas_hw"], geo) if mutant == "frame_offset_ignored" else vals
    order = select(sel_vals[:, 0], lt, mutant)
    boxes, kps = _boxes_for((case["name"], b, geo), order, table, vals)
    keep = greedy_nms(boxes, K, bound, mutant)
    n = len(keep)
    out = dict(count=n, boxes=np.zeros((K, 4), f32), kps=np.zeros((K, 5, 2), f32), scores=np.zeros(K, f32), anchor_idx=np.full(K, -1, np.int32))
    if n:
        out["boxes"][:n], out["kps"][:n], out["anchor_idx"][:n] = boxes[keep], kps[keep], order[keep]
        with np.errstate(over="ignore"):
            out["scores"][:n] = f32(1) / (f32(1) + np.exp(-vals[order[keep], 0].astype(f32)))
    if detail:
        out.update(order=order, keep=np.array(keep, np.int64), all_boxes=boxes)
    return out


def decode(case, mutant: Optional[str] = None):
    """the case's detections as engine.decode_heads returns them: counts [B], boxes [B, K, 4], kps [B, K, 5, 2], scores, anchor_idx"""
    B = case["heads"][0].shape[0]
    frames = [decode_frame(case, b, mutant) for b in range(B)]
    out = {k: np.stack([f[k] for f in frames]) for k in ("boxes", "kps", "scores", "anchor_idx")}
    out["counts"] = np.array([f["count"] for f in frames], np.int32)
    return out
