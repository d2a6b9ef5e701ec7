"""Planted head maps for the detection decode (gather_logits_kernel + decode_nms_kernel; not a test module).

A case is what engine.decode_heads reads and what oracle.network.decode_nms reads: `canvas_hw` (multiples of 32), `heads` = three
fp16 arrays [B, H_l, W_l, 32] (strides 8, 16, 32; per location two anchors of 15 values - logit, 4 distances, 5 x (dx, dy) - in
channels 0..14 and 15..29, channels 30 and 31 unused), `K`, `det_thresh` (a float32 value, handed to both sides as that value),
`nms_iou` and `forced`.  CASES is a fixed list; tests/test_decode_inputs.py proves with the host model alone that it reaches the
branches the kernel can get wrong, tests/test_gpu_decode_exact.py holds the kernel to reference(case) on every case.

Anchor index (the documented layout, restated here): level-major, within a level row-major over the locations, the two anchor
slots of a location adjacent: idx = start_l + 2 * (y * W_l + x) + a.

Only K detections come out, so two kinds of planted box make selection and order visible through them:
  BULK    every distance 4000 px: on these canvases (centres at most 576 px apart) any two overlap by IoU > 0.7, far over any NMS
          bound used, so the first bulk box in key order suppresses every other one;
  MARKER  a fraction of a stride wide (at most 1 x 0.5 px), placed so that the markers of ANY two anchors of a canvas are disjoint
          under the +1-pixel convention: x in [cx-3, cx-2] for slot 0 and [cx+1, cx+2] for slot 1, y in [cy-3, cy-2.5],
          [cy-1, cy-0.5], [cy+1, cy+1.5] for the levels 0, 1, 2 (cy is a multiple of 8, so the three bands never meet); against a
          bulk box a marker's IoU is below 1e-6.
So the output is the first bulk box plus the live markers in key order, and which markers appear says where the cut fell.
"""
from typing import Dict, List

import numpy as np

from oracle import network as onet

import decode_model

f16, f32 = np.float16, np.float32
STRIDES = (8, 16, 32)
CAP = 1024
QUIET = f16(-100.0)          # far below the lowest threshold used (score 0.05: logit -2.94)
BULK_PX = 4000.0


# ------------------------------------------------------------------------------------------------- layout
def level_dims(canvas_hw):
    return [(canvas_hw[0] // s, canvas_hw[1] // s) for s in STRIDES]


def level_starts(canvas_hw):
    """[start of level 0, 1, 2, anchor count]"""
    out = [0]
    for h, w in level_dims(canvas_hw):
        out.append(out[-1] + 2 * h * w)
    return out


def n_anchors(canvas_hw):
    return level_starts(canvas_hw)[3]


def anchor_slot(canvas_hw, idx):
    """anchor index -> (level, y, x, a)"""
    st = level_starts(canvas_hw)
    assert 0 <= idx < st[3]
    level = 0 if idx < st[1] else 1 if idx < st[2] else 2
    w = level_dims(canvas_hw)[level][1]
    pos, a = divmod(idx - st[level], 2)
    return level, pos // w, pos % w, a


def anchor_index(canvas_hw, level, y, x, a):
    h, w = level_dims(canvas_hw)[level]
    assert 0 <= y < h and 0 <= x < w and a in (0, 1)
    return level_starts(canvas_hw)[level] + 2 * (y * w + x) + a


# ------------------------------------------------------------------------------------------------- planting
def quiet_heads(B, canvas_hw):
    """every logit far below any threshold used, every other value zero"""
    heads = [np.zeros((B, h, w, 32), f16) for h, w in level_dims(canvas_hw)]
    for h in heads:
        h[..., 0] = h[..., 15] = QUIET
    return heads


def default_kps(idx):
    """ten landmark offsets in strides, sixteenths in [-1, 1], negative ones among them, different for neighbouring anchors"""
    return np.array([((idx * 5 + t * 3) % 33 - 16) / 16.0 for t in range(10)], f16)


def plant(heads, b, idx, logit, dist4, kps10=None):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    level, y, x, a = anchor_slot(canvas_hw, idx)
    row = heads[level][b, y, x]
    row[a * 15] = logit
    row[a * 15 + 1:a * 15 + 5] = np.asarray(dist4, f16)
    row[a * 15 + 5:a * 15 + 15] = default_kps(idx) if kps10 is None else np.asarray(kps10, f16)


def _exact16(v):
    h = f16(v)
    assert float(h) == float(v), v
    return h


def dist_of_box(canvas_hw, idx, box):
    """the four distances (in strides, exact in fp16) that put anchor idx's box at `box` = (x1, y1, x2, y2) in pixels"""
    level, y, x, _ = anchor_slot(canvas_hw, idx)
    s = STRIDES[level]
    cx, cy = x * s, y * s
    return [_exact16((cx - box[0]) / s), _exact16((cy - box[1]) / s), _exact16((box[2] - cx) / s), _exact16((box[3] - cy) / s)]


def bulk_box(canvas_hw, idx):
    level, y, x, _ = anchor_slot(canvas_hw, idx)
    s = STRIDES[level]
    return (x * s - BULK_PX, y * s - BULK_PX, x * s + BULK_PX, y * s + BULK_PX)


def marker_box(canvas_hw, idx):
    level, y, x, a = anchor_slot(canvas_hw, idx)
    s = STRIDES[level]
    x1 = x * s + (-3.0, 1.0)[a]
    y1 = y * s + (-3.0, -1.0, 1.0)[level]
    return (x1, y1, x1 + 0.25 * (1 + idx % 4), y1 + 0.25 * (1 + (idx // 4) % 2))


def plant_box(heads, b, idx, logit, box, kps10=None):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    plant(heads, b, idx, logit, dist_of_box(canvas_hw, idx, box), kps10)


def plant_bulk(heads, b, idx, logit):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    plant_box(heads, b, idx, logit, bulk_box(canvas_hw, idx))


def plant_marker(heads, b, idx, logit):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    plant_box(heads, b, idx, logit, marker_box(canvas_hw, idx))


def bits16(u):
    return np.array([u], np.uint16).view(f16)[0]


def ulps(x, n):
    """fp16 x moved by n steps of its bit pattern away from zero (n < 0: towards it)"""
    return bits16(int(np.array([x], f16).view(np.uint16)[0]) + n)


def logit_of(heads, b, idx):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    level, y, x, a = anchor_slot(canvas_hw, idx)
    return heads[level][b, y, x, a * 15]


def _case(name, canvas_hw, heads, K, det_thresh=0.5, nms_iou=0.4, forced=False, markers=None, **notes):
    return dict(name=name, canvas_hw=tuple(canvas_hw), heads=heads, K=int(K), det_thresh=f32(det_thresh), nms_iou=f32(nms_iou),
                forced=bool(forced), markers=sorted(markers or []), **notes)


SMALL, ODD, OVER, WIDE, DIGITS = (32, 32), (64, 96), (160, 160), (288, 352), (544, 576)


# ------------------------------------------------------------------------------------------------- the cases
def levels_case():
    """markers at the first and the last anchor of each level, both slots of one location, the last column and the last row of
    each level; every marker its own logit (not in index order), box and landmarks"""
    heads = quiet_heads(1, WIDE)
    st = level_starts(WIDE)
    idxs = [st[0], st[1] - 1, st[1], st[2] - 1, st[2], st[3] - 1,
            anchor_index(WIDE, 1, 5, 7, 0), anchor_index(WIDE, 1, 5, 7, 1)]
    for l, (h, w) in enumerate(level_dims(WIDE)):
        idxs += [anchor_index(WIDE, l, h // 2, w - 1, 0), anchor_index(WIDE, l, h - 1, 3, 1)]
    for j, i in enumerate(idxs):
        plant_marker(heads, 0, i, f16(1.0 + ((j * 5) % len(idxs)) * 0.125))
    return _case("levels", WIDE, heads, 32, markers=idxs)


def _cap_frame(heads, b, canvas_hw, n_cand, tied):
    """n_cand candidates, all but 3 or 5 of them bulk boxes (logits 1 .. 2 in 64 steps, many ties) spread over the canvas; the
    non-candidates include the first and the last anchor.  Markers: a leader (logit 5, high index), the lowest group and the one
    just above it:
      untied: anchor 5 at 0.25 alone at the bottom, anchor 900 at 0.5 just above;
      tied:   anchors 5, 300 and 900 at 0.25, anchor 20 at 0.5.
    Returns the markers."""
    A = n_anchors(canvas_hw)
    markers = {A - 13: f16(5.0), 5: f16(0.25), 900: f16(0.25 if tied else 0.5)}
    if tied:
        markers.update({300: f16(0.25), 20: f16(0.5)})
    skip = {0, A - 1}
    free = [i for i in range(A) if i not in markers and i not in skip]
    n_bulk = n_cand - len(markers)
    bulk = [free[p] for p in np.linspace(0, len(free) - 1, n_bulk).astype(int)]
    assert len(set(bulk)) == n_bulk
    for i in bulk:
        plant_bulk(heads, b, i, f16(1.0 + ((i * 37) % 64) / 64.0))
    for i, lg in markers.items():
        plant_marker(heads, b, i, lg)
    return list(markers)


def cap_case(name, n_cand, tied):
    heads = quiet_heads(1, OVER)
    m = _cap_frame(heads, 0, OVER, n_cand, tied)
    return _case(name, OVER, heads, 8, markers=m, n_candidates=n_cand)


def _tie_frame(heads, b, canvas_hw, lead_from=None):
    """every anchor the logit 2 (anchors from `lead_from` on one ulp higher), bulk boxes except the markers"""
    A = n_anchors(canvas_hw)
    if lead_from is None:
        markers = list(range(1020, 1028))
    else:
        cut = CAP - (A - lead_from) - 1                  # the last anchor below lead_from that survives
        markers = [cut - 1, cut, cut + 1, cut + 2, lead_from, lead_from + 4]
    for i in range(A):
        lg = ulps(f16(2.0), 1) if lead_from is not None and i >= lead_from else f16(2.0)
        (plant_marker if i in markers else plant_bulk)(heads, b, i, lg)
    return markers


def tie_cut_case():
    heads = quiet_heads(1, WIDE)
    return _case("tie_cut", WIDE, heads, 8, markers=_tie_frame(heads, 0, WIDE))


def ulp_above_4096_case():
    heads = quiet_heads(1, WIDE)
    return _case("ulp_above_4096", WIDE, heads, 8, markers=_tie_frame(heads, 0, WIDE, lead_from=4096))


def _markers_around_cut(heads, b, canvas_hw, det_thresh, span=3):
    """turn the `span` candidates on either side of the cut into markers (a box does not move its anchor's key)"""
    probe = dict(heads=heads, canvas_hw=canvas_hw, det_thresh=f32(det_thresh), nms_iou=f32(0.4), forced=False)
    lt, _ = decode_model.thresholds(probe)
    lg = decode_model.anchor_values(heads, b, canvas_hw)[:, 0]
    cand = decode_model.candidates(lg, lt)
    order = cand[np.argsort(-decode_model.keys_of(lg[cand], cand), kind="stable")]
    assert len(order) >= CAP + span
    markers = [int(i) for i in order[CAP - span:CAP + span]]
    for i in markers:
        plant_marker(heads, b, i, lg[i])
    return markers


def negative_over_cap_case():
    """score threshold 0.05 (logit -2.94): 1500 candidates at -1 and up to four ulps below it (ties in every group), the cut inside
    a tie group; the three candidates on either side of the cut are markers"""
    heads = quiet_heads(1, WIDE)
    A = n_anchors(WIDE)
    for j in range(1500):
        i = (j * 13) % A
        plant_bulk(heads, 0, i, ulps(f16(-1.0), (i * 7) % 5))
    m = _markers_around_cut(heads, 0, WIDE, 0.05)
    return _case("negative_over_cap", WIDE, heads, 8, det_thresh=0.05, markers=m)


def digits_case(name, canvas_hw, cut_idx, logit_bits):
    """the cut lands on anchor cut_idx with the logit `logit_bits`: 1023 anchors one or two ulps above it, anchors of the same logit
    only behind it, 200 anchors one ulp below.  Markers: the cut anchor, the first tie behind it, one lower anchor in front of it,
    one of the higher ones."""
    heads = quiet_heads(1, canvas_hw)
    A = n_anchors(canvas_hw)
    L = bits16(logit_bits)
    step = 97
    seq = [i for i in ((j * step) % A for j in range(A)) if i != cut_idx]
    assert len(set(seq)) == A - 1
    high, rest = seq[:CAP - 1], seq[CAP - 1:]
    ties = [i for i in rest if i > cut_idx][:40]
    tie_set = set(ties)
    low = [i for i in rest if i not in tie_set][:200]
    markers = [cut_idx, high[17]] + ([min(ties)] if ties else []) + [min(i for i in low)]
    for k, i in enumerate(high):
        (plant_marker if i in markers else plant_bulk)(heads, 0, i, ulps(L, 1 + k % 2))
    for i in ties + [cut_idx]:
        (plant_marker if i in markers else plant_bulk)(heads, 0, i, L)
    for i in low:
        (plant_marker if i in markers else plant_bulk)(heads, 0, i, ulps(L, -1))
    return _case(name, canvas_hw, heads, 8, markers=markers, cut_idx=cut_idx)


# boxes of the NMS cases: 20 x 20 under the +1 convention, on integer and quarter pixels
CHAIN_A, CHAIN_B, CHAIN_C = (0, 0, 19, 19), (6.25, 0, 25.25, 19), (12.5, 0, 31.5, 19)
KEEP_A, KEEP_D, KEEP_E, KEEP_F = (0, 0, 19, 19), (40, 0, 59, 19), (46, 0, 65, 19), (0, 32, 19, 51)


def _chain_frame(heads, b, canvas_hw):
    """A kills B (IoU 275/525 = 0.524); B would kill C (the same shift) but is dead; A and C overlap by 150/650 = 0.231: A and C out"""
    ia, ib, ic = (anchor_index(canvas_hw, 0, 2, x, 0) for x in (2, 3, 4))
    plant_box(heads, b, ia, f16(3.0), CHAIN_A)
    plant_box(heads, b, ib, f16(2.0), CHAIN_B)
    plant_box(heads, b, ic, f16(1.0), CHAIN_C)
    return [ia, ib, ic]


def chain_case():
    heads = quiet_heads(1, ODD)
    return _case("chain", ODD, heads, 8, nms_iou=0.4, planted=_chain_frame(heads, 0, ODD))


def second_keeper_case():
    """A and D are kept (disjoint); E overlaps D by 280/520 = 0.538 and A not at all: only the SECOND kept box suppresses it;
    F, behind E, is disjoint from all: A, D, F out"""
    heads = quiet_heads(1, ODD)
    ia, idd, ie, iff = (anchor_index(ODD, 0, 1, 1, 1), anchor_index(ODD, 0, 1, 6, 0), anchor_index(ODD, 0, 1, 7, 0), anchor_index(ODD, 1, 2, 0, 1))
    plant_box(heads, 0, ia, f16(3.0), KEEP_A)
    plant_box(heads, 0, idd, f16(2.0), KEEP_D)
    plant_box(heads, 0, ie, f16(1.0), KEEP_E)
    plant_box(heads, 0, iff, f16(0.5), KEEP_F)
    return _case("second_keeper", ODD, heads, 8, nms_iou=0.4, planted=[ia, idd, ie, iff])


def full_cap_case(name, one_short):
    """1024 candidates, K = 128.  One bulk box leads and suppresses the 896 other bulk boxes; markers (disjoint, all keepable)
    fill the rest.  kth_is_last: 126 markers + the last candidate, a marker with the lowest logit: the 128th kept box is
    candidate 1023.  one_short: 125 markers, then candidates 1022 and 1023 = the two slots of one location with the SAME box
    (IoU 1): 1022 is kept as the 127th, 1023 dies, the loop runs out with 127."""
    heads = quiet_heads(1, OVER)
    A = n_anchors(OVER)
    pair = (anchor_index(OVER, 1, 9, 9, 1), anchor_index(OVER, 1, 9, 9, 0))        # candidate 1022, candidate 1023
    n_mark = 125 if one_short else 126
    seq = [i for i in ((j * 11) % A for j in range(A)) if i not in pair]
    mark, bulk = seq[:n_mark], seq[n_mark:n_mark + 897]
    plant_bulk(heads, 0, bulk[0], f16(6.0))
    for k, i in enumerate(bulk[1:]):
        plant_bulk(heads, 0, i, f16(1.0 + (k % 48) / 16.0))
    for k, i in enumerate(mark):
        plant_marker(heads, 0, i, f16(1.0 + (k % 40) / 8.0))
    if one_short:
        plant_marker(heads, 0, pair[0], f16(0.5))
        plant_box(heads, 0, pair[1], f16(0.25), marker_box(OVER, pair[0]))
    else:
        plant_marker(heads, 0, pair[1], f16(0.25))
    return _case(name, OVER, heads, 128, markers=mark + [pair[0] if one_short else pair[1]], last_pair=pair, first_bulk=bulk[0])


def k_one_case():
    """every anchor of the canvas a candidate (1050 > cap), K = 1: the marker with the one top logit, at a high index"""
    heads = quiet_heads(1, OVER)
    A = n_anchors(OVER)
    top = A - 13
    for i in range(A):
        plant_bulk(heads, 0, i, f16(1.0 + ((i * 37) % 64) / 64.0))
    plant_marker(heads, 0, top, f16(4.0))
    return _case("k_one", OVER, heads, 1, markers=[top])


def k_cap_disjoint_case():
    """1024 candidates, all markers (pairwise disjoint), K = 128: the loop leaves at the 128th candidate"""
    heads = quiet_heads(1, OVER)
    idxs = list(range(13, 13 + CAP))
    for i in idxs:
        plant_marker(heads, 0, i, f16(1.0 + ((i * 29) % 96) / 32.0))
    return _case("k_cap_disjoint", OVER, heads, 128, markers=idxs)


IOU0_P, IOU0_Q, IOU0_R, IOU0_S = (0, 0, 10, 10), (10, 10, 20, 20), (40, 0, 50, 10), (51, 0, 60, 10)


def iou_zero_case():
    """nms_iou = 0: Q touches P by one pixel (IoU 1/241 > 0: suppressed); S is one pixel apart from R (IoU 0, not above 0: kept)"""
    heads = quiet_heads(1, ODD)
    ip, iq, ir, is_ = (anchor_index(ODD, 0, 0, 0, 0), anchor_index(ODD, 0, 1, 1, 0), anchor_index(ODD, 0, 0, 5, 1), anchor_index(ODD, 1, 0, 3, 0))
    for i, lg, box in ((ip, 3.0, IOU0_P), (iq, 2.5, IOU0_Q), (ir, 2.0, IOU0_R), (is_, 1.5, IOU0_S)):
        plant_box(heads, 0, i, f16(lg), box)
    return _case("iou_zero", ODD, heads, 8, nms_iou=0.0, planted=[ip, iq, ir, is_])


NEG0, POS0 = bits16(0x8000), bits16(0x0000)
SIGNED_ZERO = {0: NEG0, 3: NEG0, 5: POS0, 10: NEG0, 54: POS0, 100: NEG0, 200: POS0, 251: POS0}


def signed_zero_case():
    """threshold 0.5 = logit 0.0: both zeros are candidates and equal: anchor order"""
    heads = quiet_heads(1, ODD)
    for i, z in SIGNED_ZERO.items():
        plant_marker(heads, 0, i, z)
    return _case("signed_zero", ODD, heads, 16, markers=list(SIGNED_ZERO))


def signed_zero_at_the_cut_case():
    """1000 bulk boxes with positive logits, 50 markers with a zero logit (every 21st anchor; -0.0 on the lower 25, +0.0 on the
    upper 25): 1050 candidates, the cut inside the zeros: the 24 lowest-indexed zeros survive"""
    heads = quiet_heads(1, OVER)
    A = n_anchors(OVER)
    zeros = list(range(0, A, 21))
    assert len(zeros) == 50 and A == 1050
    for i in range(A):
        if i in zeros:
            plant_marker(heads, 0, i, NEG0 if zeros.index(i) < 25 else POS0)
        else:
            plant_bulk(heads, 0, i, f16(1.0 + ((i * 37) % 64) / 64.0))
    return _case("signed_zero_at_the_cut", OVER, heads, 64, markers=zeros)


def nonfinite_boxes_case():
    """in key order: Y (a NaN distance), W (plain), V (on W: suppressed), X (an inf distance), Z (plain box, a NaN landmark).  An IoU
    with Y is NaN and suppresses nothing; X's infinite area makes its IoUs 0; every value comes out as it is: Y, W, X, Z.
    Two markers with a NaN and a -inf LOGIT are no candidates in threshold mode."""
    heads = quiet_heads(1, ODD)
    iy, iw, iv, ix, iz = (anchor_index(ODD, 0, 2, 2, 0), anchor_index(ODD, 0, 2, 2, 1), anchor_index(ODD, 0, 2, 3, 0),
                          anchor_index(ODD, 1, 1, 4, 1), anchor_index(ODD, 2, 1, 1, 0))
    plant(heads, 0, iy, f16(4.0), [1.0, np.nan, 1.0, 1.0])
    plant_box(heads, 0, iw, f16(3.0), (8, 8, 27, 27))
    plant_box(heads, 0, iv, f16(2.5), (10, 8, 29, 27))
    plant(heads, 0, ix, f16(2.0), [0.5, 0.5, np.inf, 0.5])
    kz = default_kps(iz)
    kz[3] = np.nan
    plant_box(heads, 0, iz, f16(1.0), (40, 40, 50, 50), kz)
    plant_marker(heads, 0, anchor_index(ODD, 0, 6, 2, 0), np.nan)
    plant_marker(heads, 0, anchor_index(ODD, 1, 3, 5, 1), -np.inf)
    return _case("nonfinite_boxes", ODD, heads, 8, planted=[iy, iw, iv, ix, iz])


def mixed_batch_case():
    """six frames of one call on different paths: none, one candidate, exactly the cap, the tie cut (every anchor), a chain, 3000"""
    heads = quiet_heads(6, WIDE)
    A = n_anchors(WIDE)
    one = anchor_index(WIDE, 2, 8, 10, 1)                 # the last anchor
    plant_marker(heads, 1, one, f16(0.5))
    m2 = _cap_frame(heads, 2, WIDE, CAP, tied=True)
    m3 = _tie_frame(heads, 3, WIDE)
    _chain_frame(heads, 4, WIDE)
    for j in range(3000):
        i = (j * 13) % A
        plant_bulk(heads, 5, i, f16(-0.5 + ((i * 37) % 96) / 32.0))
    m5 = _markers_around_cut(heads, 5, WIDE, 0.3)
    return _case("mixed_batch", WIDE, heads, 8, det_thresh=0.3, frame_markers={1: [one], 2: m2, 3: m3, 5: m5},
                 frame_candidates=[0, 1, CAP, A, 3, 3000])


def _random_heads(rng, B, canvas_hw):
    heads = []
    for h, w in level_dims(canvas_hw):
        v = rng.standard_normal((B, h, w, 32)).astype(f32)
        v[..., 0], v[..., 15] = v[..., 0] * 3 - 1, v[..., 15] * 3 - 1
        v[..., 1:5], v[..., 16:20] = np.abs(v[..., 1:5]) * 2 + 0.5, np.abs(v[..., 16:20]) * 2 + 0.5
        v[..., 30:] = 0
        heads.append(np.round(v * 64) / 64)
    return [h.astype(f16) for h in heads]


def _set_logits(heads, b, idxs, value):
    canvas_hw = (heads[0].shape[1] * 8, heads[0].shape[2] * 8)
    for i in idxs:
        level, y, x, a = anchor_slot(canvas_hw, i)
        heads[level][b, y, x, a * 15] = value


def forced_short_case():
    """forced top-K with K = 64 above the canvas's 42 anchors: all 42 come out; NaN logits (last, by index) and -inf among them,
    a pair and a triple of equal logits"""
    heads = _random_heads(np.random.default_rng(4264), 1, SMALL)
    _set_logits(heads, 0, [3, 17, 33, 40], np.nan)
    _set_logits(heads, 0, [0, 12, 41], -np.inf)
    _set_logits(heads, 0, [30, 7], f16(1.5))
    _set_logits(heads, 0, [9, 21, 35], NEG0)
    return _case("forced_short", SMALL, heads, 64, forced=True)


def forced_mixed_case():
    """forced top-K, three frames: every logit NaN; every second anchor NaN and one +inf; ordinary"""
    heads = _random_heads(np.random.default_rng(9664), 3, ODD)
    A = n_anchors(ODD)
    _set_logits(heads, 0, range(A), np.nan)
    _set_logits(heads, 1, range(0, A, 2), np.nan)
    _set_logits(heads, 1, [197], np.inf)
    return _case("forced_mixed", ODD, heads, 16, forced=True)


def _build() -> List[Dict]:
    return [
        levels_case(),
        cap_case("cap_exact", CAP, tied=False), cap_case("cap_plus_one_unique", CAP + 1, tied=False), cap_case("cap_plus_one_tied", CAP + 1, tied=True),
        tie_cut_case(), ulp_above_4096_case(), negative_over_cap_case(),
        # the coverage condition of test_decode_inputs.py: with the cases above, these four give every (digit % 4) in every pass,
        # both halves of pass 0 and the first and the last wave of pass 2.  Pass 1's digit holds bits 12.. of 0xFFFFF - index, so
        # its values 1 and 0 (mod 4) need anchors from 8192 and from 12288 on: the one larger canvas of the list (12,852 anchors)
        digits_case("digits_a", WIDE, 3841, 0x4010), digits_case("digits_b", WIDE, 4098, 0x4020),
        digits_case("digits_c", DIGITS, 8196, 0x4030), digits_case("digits_d", DIGITS, 12291, 0x4000),
        chain_case(), second_keeper_case(),
        full_cap_case("full_cap_kth_is_last", False), full_cap_case("full_cap_one_short", True),
        k_one_case(), k_cap_disjoint_case(), iou_zero_case(),
        signed_zero_case(), signed_zero_at_the_cut_case(), nonfinite_boxes_case(),
        mixed_batch_case(), forced_short_case(), forced_mixed_case(),
    ]


CASES = _build()
for _c in CASES:
    for _h in _c["heads"]:
        _h.setflags(write=False)

POISONED = ("levels", "tie_cut", "negative_over_cap", "mixed_batch")


def case(name):
    return next(c for c in CASES if c["name"] == name)


def frame_of(c, b):
    """frame b of a case as a case of its own (B = 1)"""
    return dict(c, name=f"{c['name']}[{b}]", heads=[h[b:b + 1] for h in c["heads"]])


_REF: Dict = {}


def reference(c):
    """oracle.network.decode_nms per frame, padded to K slots as the kernel pads them (zeros, anchor -1): counts [B] int32,
    boxes [B, K, 4], kps [B, K, 5, 2], scores [B, K] float32, anchor_idx [B, K] int32.  Computed once per case; read-only."""
    if c["name"] not in _REF:
        B, K = c["heads"][0].shape[0], c["K"]
        out = dict(counts=np.zeros(B, np.int32), boxes=np.zeros((B, K, 4), f32), kps=np.zeros((B, K, 5, 2), f32),
                   scores=np.zeros((B, K), f32), anchor_idx=np.full((B, K), -1, np.int32))
        for b in range(B):
            with np.errstate(invalid="ignore", over="ignore"):
                ob, ok, osc, oa = onet.decode_nms([h[b] for h in c["heads"]], 0.0 if c["forced"] else float(c["det_thresh"]),
                                                  2.0 if c["forced"] else float(c["nms_iou"]), K)
            n = len(oa)
            out["counts"][b] = n
            out["boxes"][b, :n], out["kps"][b, :n], out["scores"][b, :n], out["anchor_idx"][b, :n] = ob, ok, osc, oa
        for arr in out.values():
            arr.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


def poison(c):
    """the case with fp16 NaN wherever the kernel has no business reading: channels 30 and 31 of every location, and the values
    1..14 of every anchor that is no candidate or falls below the cut (by decode_model's selection).  The logits stay."""
    heads = [h.copy() for h in c["heads"]]
    lt, _ = decode_model.thresholds(c)
    for h in heads:
        h[..., 30:] = np.nan
    for b in range(heads[0].shape[0]):
        live = set(int(i) for i in decode_model.select(decode_model.anchor_values(c["heads"], b, c["canvas_hw"])[:, 0], lt))
        for i in range(n_anchors(c["canvas_hw"])):
            if i not in live:
                level, y, x, a = anchor_slot(c["canvas_hw"], i)
                heads[level][b, y, x, a * 15 + 1:a * 15 + 15] = np.nan
    return dict(c, name=c["name"] + "+poison", heads=heads)
