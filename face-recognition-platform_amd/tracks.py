"""Face tracks: the numpy model of the device step that embeds a track once, not every frame (csrc/track_kernels.hip;
include/frp.h: frp_track_config).  It is the reference of every device test, and this docstring is the written form of
what the kernels do.

The workload is video: a stream's consecutive frames show the same faces in almost the same place.  A pass with
FLAG_TRACK decides on the device which detections continue a face identified before, hands the embedder only the others
and gives the rest the bits their track cached.

State, per stream: `next_id` and an ordered list of at most T = TRACK_SLOTS = 128 entries, each
    box[4] f32, id i32, age i32 (frames of this stream since the embedding the entry carries was computed),
    missed i32, match_idx i32, match_cos f32, emb[512] f32.
The model also has the handle's `stale` flag (mark_stale; the handle sets it at track_config, at every gallery mutation
and at gallery_exact): it applies to the next step as a whole and is cleared by it, so that a cached match_idx never
outlives a row move.

One frame of stream s - a stream's frames are taken in batch order, which is time order in the mixer - with detections
j = 0 .. n-1, n = clamp(counts[b], 0, K), in detector order:
  1. For j ascending, over the entries not yet claimed in this frame: IoU exactly as the NMS kernels compute it (the
     +1-pixel area form, fp32, one rounding per operation, inter / ((a + b) - inter)).  Candidates are the entries with
     iou >= iou_min (a NaN fails).  The candidate with the largest IoU is taken, on a tie the lowest entry index.
     Matched: the detection inherits `id` and gets a = age + 1; if a < refresh and the step is not stale it is REUSED: it
     carries the entry's emb / match_idx / match_cos and age = a.  Otherwise it is EMBEDDED with age 0.
     Unmatched: id = next_id++, embedded, age 0.
  2. The new list: the n detections in order with missed = 0, then the unclaimed old entries in their old order, each
     with missed + 1 and age + 1, kept only while missed <= max_missed; the list is cut at T.
A frame whose stream is -1 embeds every detection, reports track_id -1 and touches no state.  Streams that do not occur
in a batch keep their state.

The embed list is the embedded detections in frame-major (b, k) order: `face_slot` [B * K] (slot b * K + k, -1 behind
the count) and `n_embed`.  Every live slot then has emb / match_idx / match_cos - an embedded slot its own results (the
caller's emb / idx / cos arrays stand in for the embedder and the matcher), a reused slot the bits of its source, which
is an entry of the state before the step or a face embedded earlier in the same batch - and track_id, reused, age.
Slots at or beyond the count hold zero embeddings, match_idx -1, match_cos -1, track_id -1, reused 0, age 0.

The defaults (iou_min 0.3, refresh 8, max_missed 2) are ordinary defaults, not measured optima.
"""
from typing import Dict, List, Optional

import numpy as np

f32 = np.float32
TRACK_SLOTS = 128            # csrc/frp_internal.h: FRP_TRACK_SLOTS
MAX_STREAMS = 64             # include/frp.h: FRP_TRACK_MAX_STREAMS
EMB_DIM = 512
DEFAULT_IOU_MIN, DEFAULT_REFRESH, DEFAULT_MAX_MISSED = 0.3, 8, 2      # ordinary defaults, not measured optima


def check_config(iou_min, refresh, max_missed, max_streams):
    """the ranges frp_track_config accepts"""
    if not (f32(0) < f32(iou_min) <= f32(1)):
        raise ValueError("iou_min must lie in (0, 1]")
    if int(refresh) < 1 or int(max_missed) < 0 or not 1 <= int(max_streams) <= MAX_STREAMS:
        raise ValueError("refresh >= 1, max_missed >= 0, max_streams 1..64")


def iou(a, b) -> np.float32:
    """+1-pixel-area IoU of two boxes, fp32 with one rounding per operation (decode_nms_kernel's arithmetic)"""
    ax1, ay1, ax2, ay2 = (f32(v) for v in a)
    bx1, by1, bx2, by2 = (f32(v) for v in b)
    one, zero = f32(1), f32(0)
    aa = f32(f32(f32(ax2 - ax1) + one) * f32(f32(ay2 - ay1) + one))
    ba = f32(f32(f32(bx2 - bx1) + one) * f32(f32(by2 - by1) + one))
    w = np.fmax(zero, f32(f32(np.fmin(ax2, bx2) - np.fmax(ax1, bx1)) + one))      # (fmaxf / fminf: a NaN operand gives the other one)
    h = np.fmax(zero, f32(f32(np.fmin(ay2, by2) - np.fmax(ay1, by1)) + one))
    inter = f32(w * h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(inter / f32(f32(aa + ba) - inter))


class _Entry:
    __slots__ = ("box", "id", "age", "missed", "idx", "cos", "emb")

    def __init__(self, box, id_, age, missed, idx, cos, emb):
        self.box, self.id, self.age, self.missed, self.idx, self.cos, self.emb = box, id_, age, missed, idx, cos, emb


class TrackModel:
    def __init__(self, iou_min: float = DEFAULT_IOU_MIN, refresh: int = DEFAULT_REFRESH, max_missed: int = DEFAULT_MAX_MISSED,
                 max_streams: int = 1):
        check_config(iou_min, refresh, max_missed, max_streams)
        self.iou_min, self.refresh, self.max_missed, self.max_streams = f32(iou_min), int(refresh), int(max_missed), int(max_streams)
        self.next_id = [0] * self.max_streams
        self.entries: List[List[_Entry]] = [[] for _ in range(self.max_streams)]
        self.stale = True                      # as after frp_track_config
        self.embedded = self.reused = 0        # totals (frp_track_stats)

    def mark_stale(self):
        self.stale = True

    def reset(self, stream: Optional[int] = None):
        """forget the tracks of one stream, None or -1: of all"""
        for s in (range(self.max_streams) if stream is None or stream < 0 else [int(stream)]):
            self.next_id[s], self.entries[s] = 0, []

    def step(self, streams, boxes, counts, K, emb=None, idx=None, cos=None) -> Dict[str, np.ndarray]:
        """one batch.  streams [B], boxes [B, K, 4], counts [B]; emb [B, K, 512], idx, cos [B, K]: what the embedder and the
        matcher would give each slot if it is embedded (default: zeros / -1 / 0).
        -> track_id, reused, age [B, K]; face_slot [B * K], n_embed; emb, idx, cos per slot"""
        streams = np.asarray(streams, np.int32).reshape(-1)
        B, K = streams.shape[0], int(K)
        boxes = np.asarray(boxes, f32).reshape(B, K, 4)
        counts = np.asarray(counts, np.int32).reshape(B)
        if np.any(streams < -1) or np.any(streams >= self.max_streams):
            raise ValueError("a stream outside [-1, max_streams)")
        emb = np.zeros((B, K, EMB_DIM), f32) if emb is None else np.asarray(emb, f32).reshape(B, K, EMB_DIM)
        idx = np.full((B, K), -1, np.int32) if idx is None else np.asarray(idx, np.int32).reshape(B, K)
        cos = np.zeros((B, K), f32) if cos is None else np.asarray(cos, f32).reshape(B, K)
        o = dict(track_id=np.full((B, K), -1, np.int32), reused=np.zeros((B, K), np.int32), age=np.zeros((B, K), np.int32),
                 face_slot=np.full((B * K,), -1, np.int32), n_embed=0, emb=np.zeros((B, K, EMB_DIM), f32),
                 idx=np.full((B, K), -1, np.int32), cos=np.full((B, K), -1, f32))
        stale, self.stale = self.stale, False
        n_embed = 0
        for b in range(B):
            s, n = int(streams[b]), int(min(max(counts[b], 0), K))
            old = self.entries[s] if s >= 0 else []
            claimed = [False] * len(old)
            new: List[_Entry] = []
            for j in range(n):
                best, best_iou = -1, None
                for e, ent in enumerate(old):
                    if claimed[e]:
                        continue
                    v = iou(boxes[b, j], ent.box)
                    if v >= self.iou_min and (best < 0 or v.view(np.uint32) > best_iou.view(np.uint32)):      # NaN fails; ties: the lower index stays
                        best, best_iou = e, v
                ent = None
                if best >= 0:
                    claimed[best] = True
                    src = old[best]
                    a = src.age + 1
                    if a < self.refresh and not stale:
                        ent = _Entry(boxes[b, j].copy(), src.id, a, 0, src.idx, src.cos, src.emb)
                        o["reused"][b, j] = 1
                    else:
                        ent = _Entry(boxes[b, j].copy(), src.id, 0, 0, idx[b, j], cos[b, j], emb[b, j].copy())
                elif s >= 0:
                    ent = _Entry(boxes[b, j].copy(), self.next_id[s], 0, 0, idx[b, j], cos[b, j], emb[b, j].copy())
                    self.next_id[s] += 1
                else:
                    ent = _Entry(boxes[b, j].copy(), -1, 0, 0, idx[b, j], cos[b, j], emb[b, j].copy())
                if not o["reused"][b, j]:
                    o["face_slot"][n_embed] = b * K + j
                    n_embed += 1
                o["track_id"][b, j], o["age"][b, j] = ent.id, ent.age
                o["emb"][b, j], o["idx"][b, j], o["cos"][b, j] = ent.emb, ent.idx, ent.cos
                new.append(ent)
            if s < 0:
                continue
            for e, ent in enumerate(old):
                if not claimed[e] and ent.missed + 1 <= self.max_missed:
                    new.append(_Entry(ent.box, ent.id, ent.age + 1, ent.missed + 1, ent.idx, ent.cos, ent.emb))
            self.entries[s] = new[:TRACK_SLOTS]
        o["n_embed"] = n_embed
        live = int(sum(min(max(int(c), 0), K) for c in counts))
        self.embedded += n_embed
        self.reused += live - n_embed
        return o
