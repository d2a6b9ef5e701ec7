"""Planted call sequences for the face tracker (not a test module).

A case is a configuration and a list of operations on one handle / one tracks.TrackModel:
    ("step", streams [B], boxes [B, K, 4], counts [B])     one batch
    ("stale",)                                             what a gallery mutation does to the handle (TrackModel.mark_stale)
    ("reset", stream)                                      track_reset
Both sides start as frp_track_config leaves them: no tracks, stale - so the FIRST step of a case embeds every face, and
the cases that are about reuse begin with a step without detections, which only clears the flag.

stand_in(call, B, K) is what the embedder and the matcher "produce" for every slot of step number `call`: a distinct exact
pattern per (call, b, k), so that a result copied from a wrong source shows.  tests/test_tracks_host.py proves with the
model itself that each case does what it is named for; tests/test_gpu_tracks.py holds the kernels to the model on every
case, every output array, after every step.

Slots from the count on are DEAD: their boxes hold junk (finite, large) that neither side may use.
"""
from typing import Dict, List

import numpy as np

from frp_amd import tracks

f32 = np.float32
JUNK = f32(7777.0)
EMB_DIM = 512


def stand_in(call: int, B: int, K: int):
    """emb [B, K, 512], idx [B, K], cos [B, K] of step `call` (< 16; B * K < 2048): exact in fp32, distinct per (call, b, k)"""
    slot = (call * 2048 + np.arange(B * K)).astype(np.int64)
    emb = (slot[:, None] + np.arange(EMB_DIM)[None, :] / 512.0).astype(f32).reshape(B, K, EMB_DIM)
    return emb, (slot + 100000).astype(np.int32).reshape(B, K), (slot / 65536.0).astype(f32).reshape(B, K)


def _step(streams, frames, K):
    """frames: per frame the list of boxes in detector order"""
    B = len(streams)
    boxes = np.full((B, K, 4), JUNK, f32)
    counts = np.zeros((B,), np.int32)
    for b, rows in enumerate(frames):
        for j, box in enumerate(rows):
            boxes[b, j] = [f32(v) for v in box]
        counts[b] = len(rows)
    return ("step", np.asarray(streams, np.int32), boxes, counts)


def _case(name, K, ops, iou_min=0.3, refresh=8, max_missed=2, max_streams=1):
    return dict(name=name, K=int(K), ops=ops, config=dict(iou_min=iou_min, refresh=refresh, max_missed=max_missed, max_streams=max_streams))


def _prime(streams, K):
    return _step(streams, [[] for _ in streams], K)


def _shift(box, dx, dy=0.0):
    return (box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy)


FACES = [(10, 10, 50, 60), (100, 20, 150, 85), (200, 120, 230, 160)]


def batch_root_case():
    """one stream, three frames in one batch, boxes static: frame 0 is embedded, frames 1 and 2 reuse what it computes (sources are
    slots of this batch); a second batch reuses out of the table the first one stored"""
    K = 4
    return _case("batch_root", K, [_prime([0], K), _step([0, 0, 0], [FACES] * 3, K), _step([0, 0], [FACES] * 2, K)])


def two_streams_case():
    """two streams interleaved in mixer order, three calls, boxes drifting: the state persists per stream"""
    K, ops = 4, [_prime([0, 1, 0, 1], 4)]
    t = [0, 0]
    for _ in range(3):
        frames = []
        for s in (0, 1, 0, 1):
            frames.append([_shift(f, 1.5 * t[s] + 40 * s, 0.5 * t[s]) for f in (FACES if s == 0 else FACES[:2])])
            t[s] += 1
        ops.append(_step([0, 1, 0, 1], frames, K))
    return _case("two_streams", K, ops, max_streams=2)


def refresh_case():
    """refresh = 3 over seven frames of static boxes: ages 0 1 2 0 1 2 0 - the re-embed boundary, inside a batch and across two"""
    K = 3
    return _case("refresh3", K, [_prime([0], K), _step([0] * 4, [FACES[:2]] * 4, K), _step([0] * 3, [FACES[:2]] * 3, K)], refresh=3)


def missed_case():
    """max_missed = 2: face 1 is absent for 2 frames and back (kept, reused, its id), face 2 for 3 frames (dropped: a new id)"""
    K = 4
    a, b, c = FACES
    return _case("missed", K, [_prime([0], K), _step([0] * 3, [[a, b, c], [a], [a]], K), _step([0] * 3, [[a, b], [a, b, c], [a, b, c]], K)])


def greedy_tie_case():
    """frame 1: detection 0 overlaps entries 0 and 1 with EQUAL IoU bits (0.6) and takes entry 0; detection 1 then takes entry 1
    although entry 0 would have been its better match (greedy in detector order); detections 2 and 3 both overlap entry 2 only:
    the first takes it, the second gets a new id"""
    K = 4
    e0, e1, e2 = (0, 0, 19, 19), (10, 0, 29, 19), (100, 100, 139, 139)
    d = [(5, 0, 24, 19), (4, 0, 23, 19), (102, 100, 141, 139), (98, 100, 137, 139)]
    return _case("greedy_tie", K, [_prime([0], K), _step([0, 0], [[e0, e1, e2], d], K)])


def threshold_case():
    """iou_min = 0.5.  entry 0 is 9 x 18 and detection 0, 9 x 9, lies inside it: IoU = 81 / 162 = 0.5 exactly, AT the bound: matched.
    entry 1 is one fp32 step taller: IoU two fp32 steps under 0.5, just below: a new id"""
    K = 2
    tall = np.nextafter(f32(17), f32(18))
    return _case("threshold", K, [_prime([0], K), _step([0, 0], [[(0, 0, 8, 17), (100, 0, 108, tall)], [(0, 0, 8, 8), (100, 0, 108, 8)]], K)],
                 iou_min=0.5)


def gaps_case():
    """frames without detections and frames of stream -1 between a stream's frames: the empty frames age the entries (missed), the
    untracked ones embed everything with id -1 and touch nothing"""
    K = 3
    a, b, _ = FACES
    return _case("gaps", K, [_prime([0, -1], K), _step([0, -1, 0, 0, -1, 0], [[a, b], [a, b], [], [a, b], [a], [a, b]], K),
                             _step([-1, -1], [[a], []], K), _step([0, 0], [[], [b, a]], K)])


def cut_case():
    """K = 128: 128 faces, then 100 others (the list would hold 100 + 128 retained: cut at T = 128, the last 100 old entries fall out),
    then the first 128 again - 28 of them are still there and are reused, 100 get new ids.  Two static frames follow: all reused."""
    K = 128
    grid = [(30 * (i % 16), 40 * (i // 16), 30 * (i % 16) + 20, 40 * (i // 16) + 30) for i in range(128)]
    other = [_shift(g, 0, 1000) for g in grid[:100]]
    return _case("cut_at_T", K, [_prime([0], K), _step([0, 0, 0], [grid, other, grid], K), _step([0, 0], [grid, grid], K)], max_missed=3)


def stale_case():
    """a gallery change between two calls: the second embeds every face, ids and the list continue; the third reuses again"""
    K = 3
    return _case("stale", K, [_prime([0], K), _step([0, 0], [FACES] * 2, K), ("stale",), _step([0, 0], [FACES] * 2, K), _step([0], [FACES], K)])


def reset_case():
    """reset of one stream of two: stream 0 starts over at id 0 and embeds, stream 1 goes on reusing"""
    K = 3
    fr = [FACES, FACES[:2]]
    return _case("reset_one", K, [_prime([0, 1], K), _step([0, 1], fr, K), ("reset", 0), _step([0, 1, 0, 1], fr + fr, K)], max_streams=2)


def all_reused_case():
    """a batch in which nothing is embedded: n_embed = 0, every live slot carries a table entry"""
    K = 3
    return _case("all_reused", K, [_prime([0, 1], K), _step([0, 1], [FACES, FACES[1:]], K), _step([1, 0, 0, 1], [FACES[1:], FACES, FACES, FACES[1:]], K)],
                 max_streams=2)


def _build() -> List[Dict]:
    return [batch_root_case(), two_streams_case(), refresh_case(), missed_case(), greedy_tie_case(), threshold_case(), gaps_case(),
            cut_case(), stale_case(), reset_case(), all_reused_case()]


CASES = _build()
_REF = {}


def reference(case) -> List[Dict]:
    """tracks.TrackModel on the case: one entry per operation - a step's outputs, None for the others (computed once per case;
    callers must not write into it)"""
    if case["name"] not in _REF:
        m = tracks.TrackModel(**case["config"])
        outs, call = [], 0
        for op in case["ops"]:
            if op[0] == "step":
                _, streams, boxes, counts = op
                o = m.step(streams, boxes, counts, case["K"], *stand_in(call, len(streams), case["K"]))
                for v in o.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
                outs.append(o)
                call += 1
            else:
                m.mark_stale() if op[0] == "stale" else m.reset(op[1])
                outs.append(None)
        _REF[case["name"]] = (outs, m)
    return _REF[case["name"]][0]


def reference_model(case) -> tracks.TrackModel:
    """the model as the case leaves it (its totals, its final lists)"""
    reference(case)
    return _REF[case["name"]][1]
