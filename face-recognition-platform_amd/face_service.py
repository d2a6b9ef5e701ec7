"""Drop-in `FaceService` for backend/app/services/face_service.py on MI355X.

Same public surface as the reference class (methods, argument meaning, result
dict keys and their order, messages, "never raise" error convention); the
arithmetic runs in libfrp.so (HIP, gfx950) through `native.Engine`:

  reference call                                         -> here
  face_recognition.load_image_file      (:139)           -> PIL decode to RGB (host)
  face_recognition.face_locations       (:156)           -> Engine.process_frames (detector + decode/NMS)
  face_recognition.face_encodings       (:179)           -> same call (5-point warp + IResNet-100), 512-d
  np.array([ENCODINGS[t] ...]) rebuild  (:409,461,558,595)-> device-resident fp16 gallery (gallery.Gallery)
  face_recognition.face_distance        (:410,465,599)   -> Engine.match_scores / match (cosine on MFMA);
                                                            distance = sqrt(max(0, 2 - 2 cos))
Embeddings are unit vectors, so the Euclidean `distance` field, the 0.4 / 0.6
buckets (:486-492), `tolerance` (:43,411) and the sigmoid score (:497-506) keep
their meaning.  There is NO CPU fallback: without libfrp.so or a GPU the compute
methods report failure through the reference's own error convention.

New streaming entry points (fill the dead probe list at
backend/app/services/async_task_manager.py:125): process_frames / process_frame.
"""
from __future__ import annotations

import contextlib
import json
import logging
import os
import threading
import time
from collections import deque, namedtuple
from datetime import datetime
from pathlib import Path
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import ingest, lanes, native, pyramid, tracks
from .gallery import Gallery
from .mjpeg import JpegBatch
from .yuv import YuvBatch

_SOURCE_BATCHES = (JpegBatch, YuvBatch)      # batches that are not pixel arrays yet: they carry `hw` and `decode()`


def frames_hw(frames) -> Tuple[int, int]:
    """(height, width) of the frames of a batch: a source batch carries it, an array is [B, H, W, 3] or one frame [H, W, 3]"""
    return tuple(int(v) for v in (frames.hw if isinstance(frames, _SOURCE_BATCHES) else frames.shape[-3:-1]))


# What an engine can do, as this file asks it (native.Engine: all of it; the tests' partial engines: some): field -> the methods it
# stands for.  Found by duck typing, here and nowhere else; questions that sound alike and are asked differently are separate fields.
_CAPS = {
    "exact_gallery": ("gallery_exact",),             # float64 rows as enrolled behind the compat calls
    "sequence": ("sequence",),                       # the multi-call lock
    "face_quality": ("face_quality",),               # ... on the resident frames
    "match_within": ("match_within",),               # the stand-alone radius match (batch_compare_faces)
    "pass_within": ("fetch_within",),                # the radius match fused into a pass: set_within before it, fetch_within after it
    "groups": ("gallery_set_groups", "set_frame_groups"),      # gallery groups: row masks, and a pass matched under per-frame masks
    "pyramid": ("process_pyramid_resident",),        # det_scales=
    "lane": ("upload_frames_async", "swap_frames", "process_resident", "fetch_results", "sequence"),    # process_stream's overlapped form
    "stage_jpeg": ("upload_jpeg_async",),            # process_frames stages a JpegBatch: upload, swap, pass, fetch under sequence()
    "stage_yuv": ("upload_yuv_async", "swap_frames"),                                                    # ... a YuvBatch
    "track": ("track_config", "set_frame_streams", "fetch_tracks"),      # face tracks: streams=
    "cluster": ("gallery_cluster",),                 # cluster_faces' greedy sweep on the device
}
EngineCaps = namedtuple("EngineCaps", list(_CAPS))


def engine_caps(eng) -> EngineCaps:
    return EngineCaps(*(all(hasattr(eng, m) for m in methods) for methods in _CAPS.values()))


logger = logging.getLogger(__name__)

DEFAULT_TOLERANCE = float(os.getenv("FACE_TOLERANCE", "0.6"))         # face_service.py:43
DEFAULT_MODEL = os.getenv("FACE_MODEL", "hog")                        # :44 (kept as a label only)
CACHE_TTL_SECONDS = int(os.getenv("FACE_CACHE_TTL", "3600"))          # :45
BATCH_WORKERS = int(os.getenv("FACE_BATCH_WORKERS", "4"))             # :46 (batching replaces the thread pool)
BACKUP_DIR = Path(os.getenv("FACE_BACKUP_DIR", "data/backups"))       # :47
DET_THRESH = float(os.getenv("FRP_DET_THRESH", "0.5"))
NMS_IOU = float(os.getenv("FRP_NMS_IOU", "0.4"))
CLUSTER_TILE = 64          # candidate seeds scored per gallery pass in cluster_faces
MAX_FACES_ENCODE = int(os.getenv("FRP_MAX_FACES", "64"))



def enhanced_size(w: int, h: int, upscale: float = 2.0, max_pixels: int = 4_000_000) -> Tuple[int, int]:
    """the enhancer's output size (services/enhancer.py:49-62, _safe_resize_params): the frame times `upscale`, or - beyond
    `max_pixels` - scaled to that many pixels"""
    new_w = int(round(w * upscale))
    new_h = int(round(h * upscale))
    if new_w * new_h > max_pixels:
        scale = (max_pixels / (w * h)) ** 0.5
        new_w = max(1, int(round(w * scale)))
        new_h = max(1, int(round(h * scale)))
    return new_w, new_h


def enhancer_settings() -> Tuple[float, int, int, bool]:
    """(upscale factor, pixel cap, JPEG quality, sharpen) with the reference's variables, defaults and parsing (services/enhancer.py:30-33),
    read when asked"""
    return (float(os.getenv("ENHANCER_UPSCALE_FACTOR", "2")), int(os.getenv("ENHANCER_MAX_PIXELS", str(4_000_000))),
            int(os.getenv("ENHANCER_JPEG_QUALITY", "85")), os.getenv("ENHANCER_SHARPEN", "true").lower() in ("1", "true", "yes"))


_METRIC_KEYS = ("total_encodings", "total_comparisons", "cache_hits", "cache_misses",
                "cumulative_encoding_time", "cumulative_comparison_time", "failed_encodings")


def cos_to_distance(cos) -> np.ndarray:
    return np.sqrt(np.maximum(0.0, 2.0 - 2.0 * np.asarray(cos, dtype=np.float64)))


PYRAMID_PER_SCALE = 64     # det_scales: detections kept per frame and scale ahead of the cross-scale merge (Engine.process_frames_pyramid's default)
WITHIN_CAP = 64            # hit-list slots per face of the device radius match (frp.h: FRP_MAX_TOPK)


def within_min_cos(tol: float) -> float:
    """Cosine bound for the device radius match that keeps every row the host test `cos_to_distance(cos) <= tol` accepts:
    d <= tol <=> cos >= 1 - tol^2 / 2 on unit rows; taken 1e-6 lower and rounded DOWN to float32 (the device compares in float32),
    so rounding can only let extra rows through - the host re-applies `d <= tol` to what comes back.  -2 lists every row."""
    m = 1.0 - 0.5 * float(tol) * float(tol) - 1e-6
    if not m > -2.0:                      # tol >= sqrt(6) (or NaN): no cosine is excluded
        return -2.0
    return float(np.nextafter(np.float32(m), np.float32(-np.inf)))


def _f32_from_key(key: int) -> np.float32:
    """the float32 whose place in the total order -inf < ... < -0.0 < +0.0 < ... < +inf is `key` (sign-magnitude bits, unfolded)"""
    bits = key if key >= 0 else (~key) ^ 0x80000000          # key >= 0: the bit pattern itself; key < 0: a negative float, -0.0 = -1
    return np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


def cluster_min_cos(thr: float) -> float:
    """The float32 bound m of the device clustering sweep (Engine.gallery_cluster, min_cos=): for EVERY float32 cos, `cos >= m` is
    the host test `cos_to_distance(cos) <= thr` - not a bound with slack as within_min_cos, nothing re-applies the host test to
    labels.  cos_to_distance never grows with cos, so the cosines that pass are everything from one float32 upwards; that float32
    is found by bisection over the ordered bit patterns with cos_to_distance itself.  Nothing passes (thr negative or NaN): NaN,
    which no comparison reaches; everything but a NaN passes: -inf."""
    thr = float(thr)
    ok = lambda c: bool(cos_to_distance(np.float32(c)) <= thr)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = -0x7F800000 - 1, 0x7F800000          # keys of -inf and +inf
        if not ok(_f32_from_key(hi)):
            return float("nan")
        if ok(_f32_from_key(lo)):
            return float("-inf")
        while hi - lo > 1:                            # ok(lo) is false, ok(hi) true
            mid = (lo + hi) // 2
            if ok(_f32_from_key(mid)):
                hi = mid
            else:
                lo = mid
    return float(_f32_from_key(hi))


def clusters_from_seed_pos(names: List[str], seed_pos) -> Dict[str, List[str]]:
    """The reference's dict (face_service.py:552-585) from the sweep's labels: seeds arise in ascending position, so cluster k is
    the k-th seed, and a cluster lists its seed, then its members in ascending position"""
    clusters: Dict[str, List[str]] = {}
    key_of_seed: Dict[int, str] = {}
    for p, s in enumerate(np.asarray(seed_pos).tolist()):
        if s == p:
            key_of_seed[p] = f"cluster_{len(clusters)}"
            clusters[key_of_seed[p]] = [names[p]]
    for p, s in enumerate(np.asarray(seed_pos).tolist()):
        if s != p:
            clusters[key_of_seed[s]].append(names[p])
    return clusters


def within_to_matches(rows, cos, n_hits, tol: float, pos_of_row) -> List[Tuple[int, float]]:
    """One query's device hit list (Engine.match_within / fetch_within: gallery rows, float32 cosines, the true hit count) ->
    [(position, distance)] of the hits with distance <= tol, ordered by (distance, position): the order of a stable argsort
    over distances laid out by position, which is what the full-row path does.  `pos_of_row[row]` is the position of the
    row's name in the caller's target list, -1 for a row that is not among the targets."""
    n = min(int(n_hits), len(rows))
    if n <= 0:
        return []
    pos = np.asarray(pos_of_row)[np.asarray(rows[:n], dtype=np.int64)]
    d = cos_to_distance(np.asarray(cos[:n]))
    keep = (pos >= 0) & (d <= tol)
    pos, d = pos[keep], d[keep]
    order = np.lexsort((pos, d))          # last key first: by distance, ties by position
    return list(zip(pos[order].tolist(), d[order].tolist()))


def match_dicts(targets: Sequence[str], tol: float, hits=None, row=None, flag: bool = False) -> List[Dict[str, Any]]:
    """One query's list of the targets within `tol`, ascending by distance, ties in the order of `targets` (the reference sorts
    stably: face_service.py:432,479): from `hits` = [(position, distance)] as within_to_matches orders them, or from `row`, the
    distances to all targets.  flag: batch_compare_faces' form, with "match": True."""
    if hits is None:
        row = np.asarray(row)
        order = np.argsort(row, kind="stable")
        order = order[row[order] <= tol]
        hits = zip(order.tolist(), row[order].tolist())
    if flag:
        return [{"target": targets[j], "match": True, "distance": d, "confidence": confidence_level(d)} for j, d in hits]
    return [{"target": targets[j], "distance": d, "confidence": confidence_level(d)} for j, d in hits]


def face_dicts(out: Dict[str, np.ndarray], row_names: Dict[int, str], tol: float, all_matches: bool = False, names: Optional[List[str]] = None,
               hits=None, dist_rows=None, qual=None, streams=None) -> Tuple[List[List[Dict[str, Any]]], int]:
    """The fetched arrays `out` of one pass -> (per frame its list of face dicts, the number of faces).  `row_names`: gallery row -> name
    as it was under the guard; all_matches: every face gets "matches" - match_dicts of `names` from `hits` or `dist_rows` (one entry per
    face), [] when neither is given; `qual`: per face its quality dict; `streams`: the pass was tracked - one stream per frame, and `out`
    holds "track_id" / "reused": every face gets "track_id", "stream" and "tracked" (True: the result is its track's, not embedded in this
    pass).  Host arithmetic on its arguments: no device call, no lock.
    One pass of array arithmetic for the whole batch (distance, bucket, threshold), ONE tolist() per field; the per-face work left is
    building the dict (the reference builds N of them per face, camera.py:243-259)."""
    counts = np.asarray(out["counts"], dtype=np.int64)
    K = out["match_idx"].shape[1]
    live = np.arange(K)[None, :] < counts[:, None]                    # [B, K]: slots that hold a face
    rows = out["match_idx"][live].astype(np.int64)
    hit = rows >= 0
    cos = out["match_cos"][live].astype(np.float64)
    dist = cos_to_distance(cos)
    conf = np.where(dist < 0.4, "high", np.where(dist < 0.6, "medium", "low"))         # confidence_level, vectorised
    is_match = hit & (dist <= tol)
    boxes, kps, scores = out["boxes"][live].tolist(), out["kps"][live].tolist(), out["scores"][live].tolist()
    emb = out["emb"][live]                                            # [n, 512]: one gather, rows handed out as views
    rows_l, hit_l, cos_l, dist_l, conf_l, match_l = rows.tolist(), hit.tolist(), cos.tolist(), dist.tolist(), conf.tolist(), is_match.tolist()
    if streams is not None:
        tid_l, reu_l = out["track_id"][live].tolist(), out["reused"][live].tolist()
    result = []
    n = 0
    for b, c in enumerate(counts.tolist()):
        faces = []
        for i in range(n, n + c):
            h_ = hit_l[i]
            face = {"bbox": boxes[i], "kps": kps[i], "score": scores[i], "embedding": emb[i],
                    "target": row_names.get(rows_l[i]) if h_ else None,
                    "distance": dist_l[i] if h_ else None, "cosine": cos_l[i] if h_ else None,
                    "confidence": conf_l[i] if h_ else None, "match": match_l[i]}
            if all_matches:
                face["matches"] = (match_dicts(names, tol, hits=hits[i]) if hits is not None else
                                   match_dicts(names, tol, row=dist_rows[i]) if dist_rows is not None else [])
            if qual is not None:
                face["quality"] = qual[i]
            if streams is not None:
                face["track_id"], face["stream"], face["tracked"] = tid_l[i], int(streams[b]), bool(reu_l[i])
            faces.append(face)
        n += c
        result.append(faces)
    return result, n


def confidence_level(distance: float) -> str:                         # :486-492
    return "high" if distance < 0.4 else ("medium" if distance < 0.6 else "low")


def calibrate_confidence(distance: float) -> float:                   # :497-506
    x = max(0.0, min(1.0, 1.0 - distance))
    return round(float(100.0 / (1.0 + np.exp(-12.0 * (x - 0.5)))), 2)


def box_to_location(box, h: int, w: int) -> Tuple[int, int, int, int]:
    """(x1,y1,x2,y2) float -> (top,right,bottom,left) ints clipped to the image, the
    face_recognition css order the reference passes around (face_service.py:252,
    routes/face.py:199-217); truncation as deepfake_utils.py:153 does with insightface boxes."""
    x1, y1, x2, y2 = (int(v) for v in box)
    return max(y1, 0), min(x2, w), min(y2, h), max(x1, 0)


def load_image_file(path: str) -> np.ndarray:
    """face_recognition.load_image_file: PIL decode -> RGB u8 [H,W,3]."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


class NullStorage:
    """Persistence hook standing in for app.utils.db (Mongo + Fernet: out of scope)."""

    def store_embedding(self, target: str, embedding: List[float]) -> bool:
        return True

    def delete(self, target: str) -> int:
        return 0

    def has(self, target: str) -> bool:
        return True

    def ping(self) -> None:
        return None


class _Plan(NamedTuple):
    """what one frame pass asks of the engine: decided once per call (FaceService._plan), ahead of the route's branch"""
    max_faces: int
    tol: float                               # min(service tolerance, threshold)
    det_thresh: float
    flags: int                               # FLAG_NO_MATCH on an empty gallery, FLAG_WITHIN when `within`
    scales: Optional[Tuple[float, ...]]      # det_scales, checked; None: at native size only
    within: bool                             # the radius match is armed: set_within before the pass, fetch_within after it
    list_all: bool                           # all_matches on a gallery that has rows
    quality: bool
    groups: Optional[Tuple[int, ...]] = None # one mask per frame (FLAG_GROUPS is in flags): set_frame_groups before the pass
    streams: Optional[Tuple[int, ...]] = None  # one track stream per frame (FLAG_TRACK is in flags): set_frame_streams before, fetch_tracks after


BLOCKING, STAGED, OVERLAPPED = "blocking", "staged", "overlapped"


def _route(caps: EngineCaps, frames, overlapped: bool) -> str:
    """how a batch gets onto the device.  OVERLAPPED: process_stream's lane form (its caller found caps.lane); STAGED: a source batch on
    an engine that decodes / converts it on the way; BLOCKING: one process call on host pixels (a source batch is decoded here first)"""
    if overlapped:
        return OVERLAPPED
    if (isinstance(frames, JpegBatch) and caps.stage_jpeg) or (isinstance(frames, YuvBatch) and caps.stage_yuv):
        return STAGED
    return BLOCKING


def _check_det_scales(caps: EngineCaps, det_scales) -> Optional[Tuple[float, ...]]:
    """det_scales as a tuple of floats, or None; ValueError before anything reaches the engine"""
    if det_scales is None:
        return None
    try:
        scales = tuple(float(s) for s in det_scales)
    except TypeError:
        raise ValueError("det_scales must be a sequence of 1 to 4 scales") from None
    if not 1 <= len(scales) <= 4:
        raise ValueError(f"det_scales must hold 1 to 4 scales, not {len(scales)}")
    if not all(0.0 < s <= 2.0 for s in scales):          # (NaN fails the comparison too)
        raise ValueError(f"det_scales must lie in (0, 2]: {scales}")
    if len(scales) * PYRAMID_PER_SCALE > 512:
        raise ValueError("det_scales: more than 512 candidates per frame")
    if not caps.pyramid:
        raise ValueError("det_scales needs an engine with process_pyramid_resident")
    return scales


def _frame_groups(caps: EngineCaps, groups, n_frames: int) -> Optional[Tuple[int, ...]]:
    """groups= of a frame pass as one mask per frame, or None; ValueError before anything reaches the engine"""
    if groups is None:
        return None
    g = np.asarray(groups, dtype=np.uint64)
    masks = (int(g),) * n_frames if g.ndim == 0 else tuple(int(m) for m in g.reshape(-1))
    if len(masks) != n_frames:
        raise ValueError(f"groups: one mask per frame ({n_frames}), not {len(masks)}")
    if any(m > native.GROUPS_ALL for m in masks):
        raise ValueError("groups: masks have 32 bits")
    if not caps.groups:
        raise ValueError("groups needs an engine with gallery groups (set_frame_groups)")
    return masks


def _frame_streams(caps: EngineCaps, streams, n_frames: int, all_matches, groups, det_scales) -> Tuple[int, ...]:
    """streams= of a frame pass as one stream per frame; ValueError before anything reaches the engine"""
    if all_matches or groups is not None or det_scales is not None:
        raise ValueError("streams does not combine with all_matches, groups or det_scales")
    try:
        ids = tuple(int(v) for v in streams)
    except TypeError:
        raise ValueError("streams: one stream index per frame") from None
    if len(ids) != n_frames:
        raise ValueError(f"streams: one stream per frame ({n_frames}), not {len(ids)}")
    if any(v < -1 for v in ids):
        raise ValueError("streams: indices are >= 0, or -1 for a frame that is not tracked")
    if not caps.track:
        raise ValueError("streams needs an engine with face tracks (track_config)")
    return ids


def _n_frames(frames) -> int:
    if isinstance(frames, _SOURCE_BATCHES):
        return len(frames)
    return 1 if frames.ndim == 3 else int(frames.shape[0])


def _bring_in(eng, frames, staged: Optional[dict] = None) -> None:
    """the batch into the engine's resident frames through its staging buffer; `staged`: the lane's note of what is staged already"""
    if staged is None or staged.pop("key", None) != id(frames):
        ingest.stage_on(eng, frames)
    eng.swap_frames()


def _run_resident(eng, plan: _Plan, hw: Tuple[int, int]) -> None:
    """the asynchronous pass on the resident frames of size `hw`: at native size, or the pyramid of plan.scales"""
    if plan.scales is None:
        eng.process_resident(plan.max_faces, det_thresh=plan.det_thresh, nms_iou=NMS_IOU, flags=plan.flags)
    else:
        eng.process_pyramid_resident([pyramid.scaled_size(hw[0], hw[1], s) for s in plan.scales], per_scale=PYRAMID_PER_SCALE,
                                     max_faces=plan.max_faces, det_thresh=plan.det_thresh, nms_iou=NMS_IOU, flags=plan.flags)


class FaceService:
    def __init__(self, engine: Optional[Any] = None, storage: Optional[Any] = None, device: Optional[int] = None,
                 weights_blob: Optional[bytes] = None, second_engine: Optional[Any] = None):
        self.tolerance = DEFAULT_TOLERANCE
        self.model = DEFAULT_MODEL
        self._engine = engine
        self._engine_lock = threading.Lock()
        self._device = int(os.getenv("FRP_DEVICE", "0")) if device is None else device
        self._weights_blob = weights_blob
        self._storage = storage or NullStorage()
        self.ENCODINGS = Gallery(self._eng)
        # REST-style compat calls (compare_faces, find_k_nearest, batch_compare_faces, the duplicate scan, cluster_faces) score
        # against float64 copies of the rows AS ENROLLED (frp_gallery_exact / frp_gallery_distances): the reference's own
        # arithmetic (face_service.py:409-410), distances equal to 1e-6 - also for an exact copy (0.0), for d == tolerance, for
        # rows that are not unit vectors and for 128-d rows.  FRP_EXACT_COMPAT=0: cosines of the unit fp16 rows instead
        # (4 KB per identity less device memory; distances good to ~2e-3, 0.03 near 0).
        self._exact = os.getenv("FRP_EXACT_COMPAT", "1") != "0"
        if engine is not None and self._exact and engine_caps(engine).exact_gallery:
            engine.gallery_exact(True)
            self.ENCODINGS.exact = True
        # process_stream keeps two batches in flight on the GPU (lanes.py): a second handle with its own copy of the
        # gallery, fed by every update from the start (Gallery.add_mirror).  Created on first use, or injected (tests).
        self._engine2 = second_engine
        if second_engine is not None:
            self.ENCODINGS.add_mirror(second_engine)
        self._encoding_cache: Dict[str, Dict[str, Any]] = {}
        self._cache_ttl = CACHE_TTL_SECONDS
        self._cache_lock = threading.RLock()
        self._quality_history = deque(maxlen=1000)
        self._metrics_lock = threading.RLock()
        self._metrics = {k: (0.0 if k.startswith("cumulative") else 0) for k in _METRIC_KEYS}
        self._comparison_history = deque(maxlen=5000)
        self._last_detection = threading.local()
        # all_matches / batch_compare_faces on the device radius match (Engine.match_within, FLAG_WITHIN) where the engine has it;
        # False: the full score rows on the host (the same results; also what a face with more than WITHIN_CAP hits falls back to)
        self.use_within = True
        # cluster_faces' sweep on the device (Engine.gallery_cluster) where the engine has it; False: score tiles on the host (the
        # same clusters)
        self.use_device_cluster = True
        logger.info("FaceService initialized (model=%s, tolerance=%.3f)", self.model, self.tolerance)

    # ------------------------------------------------------------------ engine
    def _eng(self):
        """The HIP engine, created on first use (import must work on a box without a GPU;
        every compute call then fails loudly through the error convention)."""
        if self._engine is None:
            with self._engine_lock:
                if self._engine is None:
                    eng = native.Engine(self._device)
                    blob = self._weights_blob
                    if blob is None:
                        path = os.getenv("FRP_WEIGHTS")
                        if path:
                            with open(path, "rb") as f:
                                blob = f.read()
                        else:
                            from . import weights
                            logger.warning("FRP_WEIGHTS not set: using seeded synthetic weights (no pretrained pack offline)")
                            blob = weights.synthetic_blob()
                    eng.load_weights(blob)
                    self._blob_loaded = blob
                    if self._exact:
                        eng.gallery_exact(True)
                        self.ENCODINGS.exact = True
                    self._engine = eng
        return self._engine

    def _eng2(self):
        """The second lane's engine (same device, same weights).  It can only join while the gallery is empty - both
        copies of the matrix are then built from the same rows; afterwards process_stream runs on one lane."""
        if self._engine2 is None:
            eng = self._eng()
            with self._engine_lock:
                if self._engine2 is None:
                    if len(self.ENCODINGS) > 0 or getattr(self, "_blob_loaded", None) is None:
                        return None
                    e2 = native.Engine(self._device)
                    try:
                        e2.load_weights(self._blob_loaded)
                        self.ENCODINGS.add_mirror(e2)      # raises if an enrolment slipped in since the check above
                    except Exception:
                        e2.close()
                        return None
                    self._engine2 = e2
        return self._engine2

    def enable_second_lane(self) -> bool:
        """Create the second lane now (call before the watch list is loaded).  -> whether process_stream will overlap"""
        return self._eng2() is not None

    def _bump(self, key: str, by=1):
        with self._metrics_lock:
            self._metrics[key] += by

    # ------------------------------------------------------------------ encode (face_service.py:87-219)
    def _detect_and_embed(self, images: np.ndarray, rgb: bool = True, max_faces: int = MAX_FACES_ENCODE, match: bool = False):
        flags = (native.FLAG_RGB if rgb else 0) | (0 if match else native.FLAG_NO_MATCH)
        return self._eng().process_frames(images, max_faces=max_faces, det_thresh=DET_THRESH, nms_iou=NMS_IOU, flags=flags)

    @staticmethod
    def _sequence_of(eng):
        """the engine's multi-call lock (a pass and the face_quality call on its still-resident frames are one sequence)"""
        return eng.sequence() if engine_caps(eng).sequence else contextlib.nullcontext()

    def _quality_of(self, eng, frames, faces: List[Tuple[int, Tuple[int, int, int, int]]], rgb: bool) -> List[Dict[str, Any]]:
        """assess_face_quality for `faces` = [(frame index, (top, right, bottom, left))] of the batch `frames` ([B,H,W,3] in RGB or
        BGR order, or a JpegBatch / YuvBatch) that is RESIDENT on `eng`: one Engine.face_quality call for all rectangles the device takes;
        the host method on the caller's pixels for the others (a location that clipping left empty) and for an engine without
        face_quality (the tests' FakeEngine).  In the order of `faces`."""
        if not faces:
            return []
        H, W = frames_hw(frames)
        pixels = [None if isinstance(frames, _SOURCE_BATCHES) else frames]

        def on_host(b, loc):
            if pixels[0] is None:
                pixels[0] = frames.decode()
            img = pixels[0][b]
            return self.assess_face_quality(img if rgb else img[..., ::-1], loc)

        has = engine_caps(eng).face_quality
        on_dev = [has and 0 <= loc[0] < loc[2] <= H and 0 <= loc[3] < loc[1] <= W for _, loc in faces]
        sums = iter(eng.face_quality([(b, *loc) for (b, loc), ok in zip(faces, on_dev) if ok], rgb=rgb)) if any(on_dev) else None
        return [self.quality_from_sums((H, W, 3), loc, (loc[2] - loc[0]) * (loc[1] - loc[3]), next(sums)) if ok else on_host(b, loc)
                for (b, loc), ok in zip(faces, on_dev)]

    # ------------------------------------------------------------------ pictures back out (routes/camera.py:73-87,148-149)
    @staticmethod
    def _encode_enhanced(eng, rects, quality: int, optimize: bool = False) -> List[bytes]:
        """services/enhancer.py:64-92 for rectangles of the resident frames, on the device: each upscaled with BICUBIC to
        enhanced_size of its own size - only when that is larger (enhancer.py:80) - then UnsharpMask(1, 120, 3) when ENHANCER_SHARPEN
        says so, then JPEG.  optimize=False: Annex K Huffman tables, Pillow's save(quality=q); optimize=True: tables of the image's
        own, Pillow's save(quality=q, optimize=True) - the file the reference writes (enhancer.py:88)."""
        upscale, max_pixels, _, sharpen = enhancer_settings()
        sizes = []
        for _, top, right, bottom, left in rects:
            w, h = right - left, bottom - top
            new_w, new_h = enhanced_size(w, h, upscale, max_pixels)
            sizes.append((new_w, new_h) if new_w > w or new_h > h else (w, h))
        return eng.encode_jpeg_enhanced(rects, sizes, radius=1, percent=120, threshold=3, sharpen=sharpen, quality=quality, optimize=optimize)

    def snapshot_jpeg(self, frame: int = 0, quality: int = 95, enhance: bool = False, optimize: bool = False) -> Optional[bytes]:
        """the /snapshot route's cv2.imencode('.jpg', frame, [IMWRITE_JPEG_QUALITY, q]) for a frame that is RESIDENT on the engine
        (BGR, as the camera loop uploads it), encoded on the device.  enhance: the route's enhance=true branch (routes/snapshot.py:54-117)
        in front of the encoder - upscaled and sharpened as ENHANCER_UPSCALE_FACTOR / _MAX_PIXELS / _SHARPEN say, on the device too.
        optimize: Huffman tables of the image's own, PIL's save(optimize=True) - a smaller file for one more wait on the device.
        None, and a log line, when it cannot be encoded."""
        try:
            eng = self._eng()
            with self._sequence_of(eng):
                _, H, W = eng.resident_shape
                rects = [(int(frame), 0, W, H, 0)]
                return (self._encode_enhanced(eng, rects, quality, optimize) if enhance else eng.encode_jpeg(rects, quality=quality, optimize=optimize))[0]
        except Exception as e:
            logger.exception("Error encoding snapshot of frame %s: %s", frame, e)
            return None

    def enhance_snapshot(self, frame: int = 0, optimize: bool = False) -> Optional[bytes]:
        """services/enhancer.py's enhance_snapshot for a resident frame: snapshot_jpeg(enhance=True) at ENHANCER_JPEG_QUALITY.
        enhance_snapshot(frame, optimize=True) is the reference's file byte for byte (it saves with optimize=True, enhancer.py:88);
        the default writes the same pixels with the Annex K tables."""
        try:
            quality = enhancer_settings()[2]
        except Exception as e:
            logger.exception("Error reading the enhancer's settings: %s", e)
            return None
        return self.snapshot_jpeg(frame, quality=quality, enhance=True, optimize=optimize)

    def encode_frames(self, quality: int = 95, optimize: bool = False) -> List[bytes]:
        """every resident frame as a JPEG (gen_frames_from_cap's cv2.imencode per frame; mjpeg.multipart_part frames one for /feed),
        in one device call.  optimize: as in snapshot_jpeg.  [] and a log line on failure."""
        try:
            eng = self._eng()
            with self._sequence_of(eng):
                B, H, W = eng.resident_shape
                return eng.encode_jpeg([(b, 0, W, H, 0) for b in range(B)], quality=quality, optimize=optimize)
        except Exception as e:
            logger.exception("Error encoding the resident frames: %s", e)
            return []

    def face_thumbnails(self, faces: List[Tuple[int, Tuple[int, int, int, int]]], margin: float = 0.0, quality: int = 95,
                        enhance: bool = False, optimize: bool = False) -> List[bytes]:
        """JPEG crops of `faces` = [(frame index, (top, right, bottom, left))] out of the resident frames, each grown by `margin`
        times its height / width on every side and clipped to the frame; one device call.  enhance: every crop through the
        enhancer first, optimize: tables of every crop's own, both as in snapshot_jpeg.  [] and a log line on failure (a face that clipping leaves empty is one)."""
        try:
            eng = self._eng()
            with self._sequence_of(eng):
                _, H, W = eng.resident_shape
                rects = []
                for b, (top, right, bottom, left) in faces:
                    dy, dx = int(round(margin * (bottom - top))), int(round(margin * (right - left)))
                    rects.append((int(b), max(0, int(top) - dy), min(W, int(right) + dx), min(H, int(bottom) + dy), max(0, int(left) - dx)))
                if not rects:
                    return []
                return self._encode_enhanced(eng, rects, quality, optimize) if enhance else eng.encode_jpeg(rects, quality=quality, optimize=optimize)
        except Exception as e:
            logger.exception("Error encoding face thumbnails: %s", e)
            return []

    def encode_face(self, image_path_or_array, return_locations: bool = False, return_quality: bool = False) -> Dict[str, Any]:
        """return_quality: a "quality" list parallel to "encodings" - assess_face_quality of every face at its location, the pixel
        half computed on the device from the frames the pass left resident (routes/face.py:199-217 calls the two back to back)"""
        start = time.time()

        def failure(msg):
            return {"success": False, "face_count": 0, "encodings": [], "message": msg,
                    "processing_time": time.time() - start}

        try:
            is_path = isinstance(image_path_or_array, str)
            if is_path:
                cached = self._get_from_cache(image_path_or_array)
                if cached and (not return_quality or "quality" in cached):     # (an entry without quality: a miss when it is asked for)
                    self._bump("cache_hits")
                    result = {"success": True, "face_count": len(cached.get("encodings", [])),
                              "encodings": cached.get("encodings", []), "message": "Retrieved from cache",
                              "cached": True, "processing_time": time.time() - start}
                    if return_locations:
                        result["locations"] = cached.get("locations", [])
                    if return_quality:
                        result["quality"] = cached["quality"]
                    return result
                self._bump("cache_misses")
                image = load_image_file(image_path_or_array)
            elif isinstance(image_path_or_array, np.ndarray):
                image = image_path_or_array
            else:
                return failure("Invalid input type")

            t_enc = time.time()
            batch = image[None] if image.ndim == 3 else image
            with (self._sequence_of(self._eng()) if return_quality else contextlib.nullcontext()):
                out = self._detect_and_embed(batch)
                n = int(out["counts"][0])
                if n == 0:
                    self._bump("failed_encodings")
                    return failure("No faces detected in image")
                h, w = image.shape[:2]
                locations = [box_to_location(out["boxes"][0, k], h, w) for k in range(n)]
                quality = self._quality_of(self._eng(), batch, [(0, loc) for loc in locations], rgb=True) if return_quality else None
            encodings = [out["emb"][0, k].astype(np.float64) for k in range(n)]
            enc_time = time.time() - t_enc
            with self._metrics_lock:
                self._metrics["total_encodings"] += n
                self._metrics["cumulative_encoding_time"] += enc_time
            if is_path:
                entry = {"encodings": encodings, "locations": locations}
                if return_quality:
                    entry["quality"] = quality
                self._add_to_cache(image_path_or_array, entry)
            total = time.time() - start
            logger.info("Encoded %d face(s) in %.3fs (io+proc=%.3fs)", n, total, enc_time)
            result = {"success": True, "face_count": n, "encodings": encodings,
                      "message": f"Successfully encoded {n} face(s)", "processing_time": total}
            if return_locations:
                result["locations"] = locations
            if return_quality:
                result["quality"] = quality
            return result
        except Exception as e:  # never raise across the API (:209-219)
            logger.exception("Error encoding face: %s", e)
            self._bump("failed_encodings")
            return failure(f"Error encoding face: {str(e)}")

    def batch_encode_faces(self, image_paths: List[str], max_workers: int = BATCH_WORKERS, return_quality: bool = False) -> List[Dict[str, Any]]:
        """:224-246.  The reference fans paths out over a 4-thread pool (one detect+embed per image,
        results in completion order); here uncached images of equal size are stacked into ONE device
        batch (chunks of `max_workers * 8` frames) and results come back in input order.
        return_quality: as encode_face - one device quality call per chunk, on its still-resident frames."""
        start = time.time()
        results: List[Optional[Dict[str, Any]]] = [None] * len(image_paths)
        pending: Dict[Tuple[int, ...], List[Tuple[int, np.ndarray]]] = {}
        for i, path in enumerate(image_paths):
            try:
                cached = self._get_from_cache(path) if isinstance(path, str) else None
                if cached is not None and return_quality and "quality" not in cached:
                    cached = None                                # an entry without quality: a miss when it is asked for
                if cached is not None or not isinstance(path, str):
                    # cache hit / invalid input: the single-image path
                    results[i] = self.encode_face(path, return_quality=True) if return_quality else self.encode_face(path)
                    continue
                self._bump("cache_misses")
                img = load_image_file(path)
                pending.setdefault(img.shape, []).append((i, img))
            except Exception as e:
                logger.exception("Batch encode failed for %s: %s", path, e)
                self._bump("failed_encodings")
                results[i] = {"success": False, "face_count": 0, "encodings": [], "message": f"Error encoding face: {str(e)}",
                              "processing_time": time.time() - start}
        chunk = max(1, max_workers) * 8
        for shape, items in pending.items():
            for c0 in range(0, len(items), chunk):
                part = items[c0:c0 + chunk]
                t0 = time.time()
                try:
                    stack = np.stack([im for _, im in part])
                    with (self._sequence_of(self._eng()) if return_quality else contextlib.nullcontext()):
                        out = self._detect_and_embed(stack)
                        if return_quality:
                            h, w = shape[:2]
                            faces = [(bi, box_to_location(out["boxes"][bi, k], h, w)) for bi in range(len(part)) for k in range(int(out["counts"][bi]))]
                            quality = iter(self._quality_of(self._eng(), stack, faces, rgb=True))
                except Exception as e:
                    logger.exception("Batch encode failed: %s", e)
                    for i, _ in part:
                        self._bump("failed_encodings")
                        results[i] = {"success": False, "face_count": 0, "encodings": [], "message": f"Error encoding face: {str(e)}",
                                      "processing_time": time.time() - start}
                    continue
                dt = time.time() - t0
                for bi, (i, img) in enumerate(part):
                    n = int(out["counts"][bi])
                    if n == 0:
                        self._bump("failed_encodings")
                        results[i] = {"success": False, "face_count": 0, "encodings": [], "message": "No faces detected in image",
                                      "processing_time": time.time() - start}
                        continue
                    h, w = img.shape[:2]
                    locs = [box_to_location(out["boxes"][bi, k], h, w) for k in range(n)]
                    encs = [out["emb"][bi, k].astype(np.float64) for k in range(n)]
                    with self._metrics_lock:
                        self._metrics["total_encodings"] += n
                        self._metrics["cumulative_encoding_time"] += dt / len(part)
                    entry = {"encodings": encs, "locations": locs}
                    if return_quality:
                        entry["quality"] = [next(quality) for _ in range(n)]
                    self._add_to_cache(image_paths[i], entry)
                    results[i] = {"success": True, "face_count": n, "encodings": encs,
                                  "message": f"Successfully encoded {n} face(s)", "processing_time": time.time() - start}
                    if return_quality:
                        results[i]["quality"] = entry["quality"]
        for i, path in enumerate(image_paths):
            results[i]["image_path"] = path
        return results  # type: ignore[return-value]

    # ------------------------------------------------------------------ quality (:251-339), host arithmetic
    @staticmethod
    def _gray(rgb: np.ndarray) -> np.ndarray:
        # cv2.COLOR_RGB2GRAY fixed-point form: (R*4899 + G*9617 + B*1868 + 8192) >> 14
        r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
        return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)

    @staticmethod
    def _laplacian_var(gray: np.ndarray) -> float:
        # cv2.Laplacian(gray, CV_64F): 3x3 [[0,1,0],[1,-4,1],[0,1,0]], BORDER_REFLECT_101
        g = np.pad(gray.astype(np.float64), 1, mode="reflect")
        lap = g[:-2, 1:-1] + g[2:, 1:-1] + g[1:-1, :-2] + g[1:-1, 2:] - 4.0 * g[1:-1, 1:-1]
        return float(lap.var())

    @staticmethod
    def _pixel_scores(lap_var: float, mean: float, std: float) -> Tuple[float, float]:
        """(blur_score, lighting_score) from the Laplacian's variance and the grey crop's mean and standard deviation (:283-297)"""
        blur_score = min(100.0, (lap_var / 500.0) * 100.0)
        brightness = 100.0 - abs(mean - 128.0) / 128.0 * 100.0
        contrast = min(100.0, (std / 50.0) * 100.0)
        return blur_score, (brightness + contrast) / 2.0

    def assess_face_quality(self, image, face_location: Tuple[int, int, int, int]) -> Dict[str, Any]:
        top, right, bottom, left = face_location
        try:
            crop = image[top:bottom, left:right]
            if crop.size == 0 or crop.ndim != 3:
                raise ValueError("empty crop")
            gray = self._gray(crop)
            blur_score, lighting_score = self._pixel_scores(self._laplacian_var(gray), float(np.mean(gray)), float(np.std(gray)))
        except Exception as err:
            logger.debug("Blur/lighting analysis error: %s", err)
            blur_score = lighting_score = 50.0
        return self._quality_result(image.shape, face_location, blur_score, lighting_score)

    def quality_from_sums(self, shape, face_location: Tuple[int, int, int, int], n_pixels: int, sums) -> Dict[str, Any]:
        """assess_face_quality with the pixel half done on the device (Engine.face_quality): `sums` = S1, S2, L1, L2 = sum g,
        sum g^2, sum lap, sum lap^2 over the N = n_pixels grey values of the crop of an image of `shape`.  Variances as
        (N*S2 - S1^2) / N^2 with the numerator in Python integers (N*L2 passes 2^63 for a 4K crop) and ONE float64 division each:
        correctly rounded, where numpy's float64 passes over the crop are good to ~1e-13 relative."""
        n = int(n_pixels)
        s1, s2, l1, l2 = (int(v) for v in sums)
        var_g = (n * s2 - s1 * s1) / (n * n)
        var_lap = (n * l2 - l1 * l1) / (n * n)
        blur_score, lighting_score = self._pixel_scores(var_lap, s1 / n, float(np.sqrt(var_g)))
        return self._quality_result(shape, face_location, blur_score, lighting_score)

    def _quality_result(self, shape, face_location, blur_score: float, lighting_score: float) -> Dict[str, Any]:
        """the geometry terms (:257-275), the weighted score, the issue list and the history entry of one assessment"""
        top, right, bottom, left = face_location
        height, width = shape[:2]
        fw, fh = max(1, right - left), max(1, bottom - top)
        size_ratio = float(fw * fh) / float(width * height) if width * height > 0 else 0.0
        size_score = min(100.0, (size_ratio / 0.25) * 100.0)
        cx, cy = (left + right) / 2.0, (top + bottom) / 2.0
        off = np.sqrt(((cx - width / 2.0) / width) ** 2 + ((cy - height / 2.0) / height) ** 2) if width and height else 0.0
        position_score = max(0.0, (1.0 - off) * 100.0)
        aspect_ratio = min(fw, fh) / max(fw, fh)
        aspect_score = aspect_ratio * 100.0
        overall = size_score * 0.25 + position_score * 0.2 + aspect_score * 0.2 + blur_score * 0.2 + lighting_score * 0.15
        issues: List[str] = []
        if size_ratio < 0.05:
            issues.append("Face too small - move closer or crop image")
        if size_ratio > 0.8:
            issues.append("Face too large - image should show some background")
        if off > 0.4:
            issues.append("Face not centered - adjust framing")
        if aspect_ratio < 0.75:
            issues.append("Face appears distorted or at extreme angle")
        if blur_score < 40:
            issues.append("Image is blurry - use better focus or steady camera")
        if lighting_score < 40:
            issues.append("Poor lighting - improve lighting conditions")
        self._quality_history.append({"timestamp": datetime.now().isoformat(), "score": overall,
                                      "blur_score": blur_score, "lighting_score": lighting_score})
        return {"score": round(overall, 2), "size_score": round(size_score, 2), "position_score": round(position_score, 2),
                "aspect_score": round(aspect_score, 2), "blur_score": round(blur_score, 2),
                "lighting_score": round(lighting_score, 2), "issues": issues}

    # ------------------------------------------------------------------ gallery distances
    def _distances(self, encoding, names: Optional[List[str]] = None) -> Tuple[List[str], np.ndarray]:
        """names (dict order) and their distances to `encoding`: one device pass over the gallery."""
        G = self.ENCODINGS
        with G.locked():           # names, device rows and the score row belong to ONE gallery state
            targets = G.names() if names is None else [t for t in names if t in G]
            if not targets:
                return [], np.zeros((0,))
            if G.exact:            # float64 Euclidean distances to the rows as enrolled (face_recognition.face_distance, :410)
                d = self._eng().gallery_distances(np.asarray(encoding, dtype=np.float64).reshape(1, -1))[0]
                return targets, d[G.rows_of(targets)]
            q = np.asarray(encoding, dtype=np.float32).reshape(1, -1)
            cos = self._eng().match_scores(q)[0]
            return targets, cos_to_distance(cos[G.rows_of(targets)])

    # ------------------------------------------------------------------ store / delete (:344-390, :517-547)
    def store_face(self, target_name: str, encoding: np.ndarray, groups: Optional[int] = None) -> Dict[str, Any]:
        """:344-390.  groups: the identity's group mask (Gallery.put).  The exclusive gallery lock (which stalls every streaming lane) is held for the duplicate scan and for
        the insert only; the storage write (DB round trip) and the on-disk backup run outside it, in the reference's order:
        scan -> store_embedding -> ENCODINGS[name] = ... -> backup."""
        try:
            enc = np.asarray(encoding, dtype=np.float64).reshape(-1)
            is_dup, similar = False, None
            with self.ENCODINGS.locked():          # scan and `already` against ONE gallery state
                if len(self.ENCODINGS):
                    names, d = self._distances(enc)
                    for n, dist in zip(names, d):          # first hit in dict order, as :353-364
                        if n != target_name and dist < 0.3:
                            is_dup, similar = True, n
                            logger.warning("Potential duplicate: %s ~ %s (distance=%.3f)", target_name, n, dist)
                            break
            if not self._storage.store_embedding(target_name, enc.tolist()):
                return {"success": False, "message": "Failed to store in database", "is_duplicate": is_dup}
            already = self.ENCODINGS.put(target_name, enc, **({} if groups is None else {"groups": groups}))     # exclusive inside; reaches every lane's copy
            try:
                self._backup_encoding_atomic(target_name, enc.tolist())
            except Exception as be:
                logger.warning("Backup failed for %s: %s", target_name, be)
            message = f"Face {'updated' if already else 'stored'} successfully for '{target_name}'"
            if is_dup:
                message += f" (Warning: Similar to '{similar}')"
            return {"success": True, "message": message, "is_duplicate": is_dup,
                    "similar_to": similar if is_dup else None, "was_update": already}
        except Exception as e:
            logger.exception("Error storing face %s: %s", target_name, e)
            return {"success": False, "message": f"Error storing face: {str(e)}", "is_duplicate": False}

    def delete_face(self, target_name: str) -> Dict[str, Any]:
        try:
            removed_mem = self.ENCODINGS.remove(target_name)
            self._remove_from_cache(target_name)
            removed_db = self._storage.delete(target_name) > 0
            try:
                bp = BACKUP_DIR / f"{target_name}_backup.json"
                if bp.exists():
                    bp.unlink()
            except Exception:
                logger.debug("Failed to remove backup for %s (non-fatal)", target_name)
            if removed_mem or removed_db:
                return {"success": True, "message": f"Face '{target_name}' deleted successfully",
                        "removed_from_memory": removed_mem, "removed_from_db": removed_db}
            return {"success": False, "message": f"Face '{target_name}' not found in database or memory"}
        except Exception as e:
            logger.exception("Error deleting face %s: %s", target_name, e)
            return {"success": False, "message": f"Error deleting face: {str(e)}"}

    def get_all_targets(self) -> List[str]:
        return self.ENCODINGS.names()

    # ------------------------------------------------------------------ compare (:395-443)
    def compare_faces(self, test_encoding: np.ndarray, target_names: Optional[List[str]] = None,
                      return_distances: bool = True) -> List[Dict[str, Any]]:
        start = time.time()
        try:
            targets, distances = self._distances(test_encoding, target_names)
            if not targets:
                logger.warning("No targets available for comparison")
                return []
            tol = self.tolerance
            now = datetime.now().isoformat
            results: List[Dict[str, Any]] = []
            for target, d in zip(targets, distances.tolist()):
                is_match = d <= tol
                item = {"target": target, "match": is_match}
                if return_distances:
                    item["distance"] = d
                    item["confidence"] = confidence_level(d)
                    item["confidence_score"] = calibrate_confidence(d)
                results.append(item)
                self._comparison_history.append({"distance": d, "match": is_match, "timestamp": now()})
            if return_distances:
                results.sort(key=lambda x: x.get("distance", 1.0))
            with self._metrics_lock:
                self._metrics["total_comparisons"] += len(targets)
                self._metrics["cumulative_comparison_time"] += time.time() - start
            return results
        except Exception as e:
            logger.exception("Error comparing faces: %s", e)
            return []

    def batch_compare_faces(self, test_encodings: List[np.ndarray], target_names: Optional[List[str]] = None):
        """:448-481 -- one device GEMM for all queries instead of a Python loop over them."""
        G = self.ENCODINGS
        if len(test_encodings) == 0:
            return []
        tol = self.tolerance
        hits = None
        try:
            with G.locked():
                targets = G.names() if target_names is None else [t for t in target_names if t in G]
                if not targets:
                    return [[] for _ in test_encodings]
                eng = self._eng()
                if G.exact:
                    Q = np.stack([np.asarray(q, dtype=np.float64).reshape(-1) for q in test_encodings])
                    D = eng.gallery_distances(Q)[:, G.rows_of(targets)]
                else:
                    Q = np.stack([np.asarray(q, dtype=np.float32).reshape(-1) for q in test_encodings])
                    hits = self._within_hits(self.use_within and engine_caps(eng).match_within, targets, tol,
                                             lambda: eng.match_within(Q, within_min_cos(tol), WITHIN_CAP))
                    if hits is None:
                        D = cos_to_distance(eng.match_scores(Q)[:, G.rows_of(targets)])
        except Exception as e:
            logger.exception("Error in batch comparison: %s", e)
            return [[] for _ in test_encodings]
        if hits is not None:
            return [match_dicts(targets, tol, hits=hl, flag=True) for hl in hits]
        return [match_dicts(targets, tol, row=d, flag=True) for d in D]

    def _pos_of_row(self, targets: List[str]) -> Optional[np.ndarray]:
        """gallery row -> position in `targets` (-1: not a target); None when a name is listed twice (a row then has two positions)"""
        G = self.ENCODINGS
        rows = G.rows_of(targets)
        pos = np.full(len(G), -1, dtype=np.int64)
        pos[rows] = np.arange(len(rows))
        return pos if int((pos >= 0).sum()) == len(rows) else None

    def _within_hits(self, armed: bool, targets: List[str], tol: float, lists: Callable[[], Tuple[np.ndarray, np.ndarray, np.ndarray]]):
        """per query [(position in targets, distance)] within tol from the device radius match: `lists()` -> (idx [M, cap], cos [M, cap],
        n_hits [M]), one hit list per query (Engine.match_within, or Engine.fetch_within cut down to the slots that hold a face).
        None: not on this path - `armed` is off (switched off, or an engine without it; lists() is not called then), a name listed
        twice, or a query with more hits than a list holds (the reference lists every target, so a list may not be cut): the caller
        takes the full score rows.  Gallery lock held."""
        if not armed:
            return None
        pos_of_row = self._pos_of_row(targets)
        if pos_of_row is None:
            return None
        idx, cos, n_hits = lists()
        if int(n_hits.max(initial=0)) > WITHIN_CAP:
            return None
        return [within_to_matches(r, c, k, tol, pos_of_row) for r, c, k in zip(idx, cos, n_hits)]

    def _get_confidence_level(self, distance: float) -> str:
        return confidence_level(distance)

    def _calibrate_confidence(self, distance: float) -> float:
        return calibrate_confidence(distance)

    # ------------------------------------------------------------------ clustering / k-NN (:552-612)
    def cluster_faces(self, distance_threshold: float = 0.6) -> Dict[str, List[str]]:
        G = self.ENCODINGS
        with G.locked():
            if len(G) < 2:
                return {"cluster_0": G.names()}
            names = G.names()
            rows = G.rows_of(names)
            if self.use_device_cluster and engine_caps(self._eng()).cluster:
                # the whole sweep in one call: rows, score tiles and labels stay on the device, one int per name comes back
                bound = {"max_dist": float(distance_threshold)} if G.exact else {"min_cos": cluster_min_cos(distance_threshold)}
                seed_pos, _ = self._eng().gallery_cluster(rows, tile=min(CLUSTER_TILE, 64), **bound)
                return clusters_from_seed_pos(names, seed_pos)
            emb = self._eng().gallery_get_exact()[rows] if G.exact else self._eng().gallery_get().astype(np.float32)[rows]
            clusters: Dict[str, List[str]] = {}
            assigned = np.zeros(len(names), dtype=bool)
            cid = 0
            # N x N on the device: the seeds of one greedy sweep are not known up front (a member never becomes
            # a seed), so score rows are produced in tiles of CLUSTER_TILE candidate seeds per gallery pass
            # (one frp_match_scores GEMM each) instead of one pass per seed
            tile_rows: Dict[int, int] = {}
            tile = None
            for i, name in enumerate(names):           # greedy seed order = dict order, as the reference
                if assigned[i]:
                    continue
                if i not in tile_rows:                 # next tile: the first CLUSTER_TILE unassigned names from i on
                    cand = [j for j in range(i, len(names)) if not assigned[j]][:CLUSTER_TILE]
                    tile_rows = {j: t for t, j in enumerate(cand)}
                    tile = (self._eng().gallery_distances(emb[cand])[:, rows] if G.exact
                            else cos_to_distance(self._eng().match_scores(emb[cand])[:, rows]))
                d = tile[tile_rows[i]]
                take = (~assigned) & (d <= distance_threshold)
                take[i] = True
                members = [name] + [names[j] for j in np.nonzero(take)[0] if j != i]
                assigned |= take
                clusters[f"cluster_{cid}"] = members
                cid += 1
            return clusters

    def find_k_nearest(self, test_encoding: np.ndarray, k: int = 5) -> List[Dict[str, Any]]:
        """face_service.py:590-612 with the distance pass AND the k-selection on the device (ties: the
        earlier gallery row first; the reference's argpartition leaves tie order unspecified)."""
        n = len(self.ENCODINGS)
        if n == 0:
            return []
        k = min(int(k), n)
        if k < 1:
            return []
        if self.ENCODINGS.exact or k > native.MAX_TOPK:   # exact rows (or k beyond the device limit): full distance row + host selection
            targets, distances = self._distances(test_encoding)
            idx = np.argsort(distances, kind="stable")[:k]
            pairs = [(targets[int(i)], float(distances[int(i)])) for i in idx]
        else:
            q = np.asarray(test_encoding, dtype=np.float32).reshape(1, -1)
            with self.ENCODINGS.locked():      # rows -> names against the gallery state the match saw
                rows, cos = self._eng().match(q, topk=k)
                rows, cos = np.atleast_2d(rows)[0], np.atleast_2d(cos)[0]
                pairs = [(self.ENCODINGS.name_of_row(int(r)), float(cos_to_distance(float(c)))) for r, c in zip(rows, cos) if r >= 0]
        return [{"target": t, "distance": d, "confidence": confidence_level(d),
                 "confidence_score": calibrate_confidence(d)} for t, d in pairs]

    # ------------------------------------------------------------------ streaming entry points (new)
    def process_frames(self, frames_bgr: np.ndarray, max_faces: int = 10, threshold: Optional[float] = None,
                       det_thresh: Optional[float] = None, all_matches: bool = False, quality: bool = False,
                       det_scales: Optional[Sequence[float]] = None, groups=None, streams=None) -> List[List[Dict[str, Any]]]:
        """The live-loop body of routes/camera.py:225-259 for a batch of BGR frames, with the
        per-face compare + filter reduced to a fused device top-1: per frame a list of
        {bbox, kps, score, embedding, target, distance, cosine, confidence, match}.
        all_matches=True additionally lists EVERY enrolled target within both the service
        tolerance and `threshold` (the reference's exact loop semantics, camera.py:246-256: a face
        can hit several near-duplicate identities), ascending by distance, under "matches".
        quality=True adds "quality" to every face: assess_face_quality (the reference's enrolment gate, routes/face.py:217) of the
        frame at box_to_location(bbox), the pixel half from the batch's still-resident frames in one device call.
        det_scales=(1.0, 0.5, ...) detects at those scales of every frame (the `det_size` of an anchor-dense detector: a 4K camera
        detects at half size), merges the scales on the device and embeds from the full-resolution frames - one device pass
        (Engine.process_pyramid_resident); 1 to 4 scales, each in (0, 2].  None: at native size only.
        groups=[mask per frame] (or one int for all): gallery groups - the faces of frame b are matched against the enrolled
        identities whose mask shares a bit with groups[b] only (store_face(..., groups=), Gallery.set_groups): "target" is the best
        PERMITTED identity and "matches" lists permitted ones, as if the gallery held nothing else; mask 0 matches nobody.
        streams=[stream index per frame] (configure_tracks first): face tracks - the frames of a stream are consecutive frames of one
        camera, in batch order; a face that continues a track identified before is not embedded again but carries its track's result
        (tracks.TrackModel has the rules).  Every face dict gains "track_id", "stream" and "tracked" (True: a reused result); -1 marks
        a frame that is not tracked.  Not together with all_matches, groups or det_scales (ValueError)."""
        return self._process_frames_on(self._eng(), self.ENCODINGS.locked(), frames_bgr, max_faces, threshold, det_thresh, all_matches,
                                       quality=quality, det_scales=det_scales, groups=groups, streams=streams)

    def _process_frames_on(self, eng, guard, frames, max_faces, threshold, det_thresh, all_matches, take_next=None, staged=None,
                           quality=False, det_scales=None, groups=None, streams=None):
        """One frame pass on `eng`.  `take_next` / `staged` (process_stream on an engine with the lane calls): the overlapped form - this
        batch goes to the device through the engine's staging buffer (already there when the previous call staged it), the batch the
        lane will get next is claimed and its upload started on the copy stream while this batch's kernels run."""
        caps = engine_caps(eng)
        frame_streams = _frame_streams(caps, streams, _n_frames(frames), all_matches, groups, det_scales) if streams is not None else None
        scales = _check_det_scales(caps, det_scales)
        frame_groups = _frame_groups(caps, groups, _n_frames(frames)) if groups is not None else None
        if isinstance(frames, YuvBatch):
            frames.validate()                                          # (an odd size, mixed geometry: before anything reaches the engine)
        route = _route(caps, frames, take_next is not None and staged is not None)
        if route == OVERLAPPED:
            _bring_in(eng, frames, staged)                             # (ahead of the guard: the lane owns its staging buffer)
        G = self.ENCODINGS
        # The device returns gallery ROW indices; store/delete move rows (swap-remove).  The guard (exclusive for
        # process_frames, shared between the lanes of process_stream) is held over the device call and the
        # row -> name snapshot, so a concurrent delete can neither mis-attribute a face to the identity that was
        # moved into its row nor shrink the table under the lookup.
        with guard:
            plan = self._plan(caps, len(G) > 0, max_faces, threshold, det_thresh, all_matches, quality, scales, frame_groups, frame_streams)
            if plan.within:
                eng.set_within(within_min_cos(plan.tol), WITHIN_CAP)
            if plan.groups is not None:
                eng.set_frame_groups(plan.groups)
            if plan.streams is not None:
                eng.set_frame_streams(plan.streams)
            if route == OVERLAPPED:
                out, qual = self._overlapped_pass(eng, frames, plan, take_next, staged)
            elif route == STAGED:
                with eng.sequence():
                    _bring_in(eng, frames)
                    _run_resident(eng, plan, frames_hw(frames))
                    out, qual = self._fetch(eng, frames, plan)
            else:
                out, qual = self._blocking_pass(eng, frames, plan)
            n_gallery = len(G)
            row_names = {int(r): G.name_of_row(int(r)) for r in np.unique(out["match_idx"]) if r >= 0}
            listed = self._all_matches_of(eng, out, plan) if plan.list_all and int(out["counts"].sum()) > 0 else {}

        def finish():
            result, n = face_dicts(out, row_names, plan.tol, all_matches, qual=qual, streams=plan.streams, **listed)
            with self._metrics_lock:
                self._metrics["total_encodings"] += n
                self._metrics["total_comparisons"] += n * n_gallery
            return result

        # process_stream: the dicts of this batch are built by the lane's thread while its NEXT batch is on the device
        # (lanes.Deferred); everything they need was taken above, under the guard.
        return lanes.Deferred(finish) if route == OVERLAPPED else finish()

    def _plan(self, caps: EngineCaps, have_gallery: bool, max_faces, threshold, det_thresh, all_matches, quality, scales,
              frame_groups=None, frame_streams=None) -> "_Plan":
        tol = self.tolerance if threshold is None else min(self.tolerance, threshold)   # camera.py:250
        list_all = bool(all_matches) and have_gallery
        # all_matches on the device: the pass's own match kernel also lists every row within the bound (FLAG_WITHIN)
        within = bool(list_all and self.use_within and caps.pass_within)
        flags = (0 if have_gallery else native.FLAG_NO_MATCH) | (native.FLAG_WITHIN if within else 0)
        groups = frame_groups if have_gallery else None          # (an empty gallery: FLAG_NO_MATCH, which the grouped pass refuses)
        if groups is not None:
            flags |= native.FLAG_GROUPS
        if frame_streams is not None:
            flags |= native.FLAG_TRACK
        return _Plan(max_faces, tol, DET_THRESH if det_thresh is None else det_thresh, flags, scales, within, list_all, bool(quality), groups,
                     frame_streams)

    def _overlapped_pass(self, eng, frames, plan: "_Plan", take_next, staged):
        """what only the lane form does, between the shared steps: stage the lane's next batch and build the PREVIOUS one's dicts (idle)"""
        _run_resident(eng, plan, frames_hw(frames))                    # asynchronous
        nxt = take_next()
        if nxt is not None:
            ingest.stage_on(eng, nxt)                                  # copy stream: under this batch's kernels
            staged["key"] = id(nxt)
        idle = getattr(take_next, "idle", None)
        if idle is not None:
            idle()
        return self._fetch(eng, frames, plan)                          # (quality: before the lane's next swap_frames)

    def _fetch(self, eng, frames, plan: "_Plan"):
        """-> (the results of the queued pass - waits for it -, the quality list of its faces while the frames are still resident, or None)"""
        out = eng.fetch_results()
        if plan.streams is not None:
            out.update(eng.fetch_tracks())
        return out, (self._stream_quality(eng, frames, out) if plan.quality else None)

    def _blocking_pass(self, eng, frames, plan: "_Plan"):
        """the pass as ONE engine call on host pixels -> (results, quality list or None)"""
        if isinstance(frames, _SOURCE_BATCHES):
            frames = frames.decode()                                   # an engine without the device decoder / converter (tests' FakeEngine)
        kw = dict(max_faces=plan.max_faces, det_thresh=plan.det_thresh, nms_iou=NMS_IOU, flags=plan.flags)
        with (self._sequence_of(eng) if plan.quality or plan.streams is not None else contextlib.nullcontext()):
            if plan.scales is None:
                out = eng.process_frames(frames, **kw)
                if plan.streams is not None:
                    out.update(eng.fetch_tracks())
            else:
                out = eng.process_frames_pyramid(frames, scales=plan.scales, per_scale=PYRAMID_PER_SCALE, on_device=True, **kw)
            return out, (self._stream_quality(eng, frames, out) if plan.quality else None)

    def _all_matches_of(self, eng, out, plan: "_Plan") -> Dict[str, Any]:
        """face_dicts' `names` and `hits` or `dist_rows` for the faces of `out`: the hit lists of the pass where the radius match was
        armed and no list was cut, else one full-row pass over the gallery.  Gallery guard held."""
        G = self.ENCODINGS
        names = G.names()
        counts = np.asarray(out["counts"])

        def lists():
            idx, cos, n_hits = eng.fetch_within()
            live = np.arange(n_hits.shape[1])[None, :] < counts[:, None]
            return idx[live], cos[live], n_hits[live]

        hits = self._within_hits(plan.within, names, plan.tol, lists)
        if hits is not None:
            return {"names": names, "hits": hits}
        Q = np.concatenate([out["emb"][b, :int(c)] for b, c in enumerate(counts)])
        dist = cos_to_distance(eng.match_scores(Q)[:, G.rows_of(names)])
        if plan.groups is not None:            # the score rows ignore groups: identities the face's frame does not permit are beyond any tolerance
            face_mask = np.repeat(np.asarray(plan.groups, np.uint32), np.minimum(counts, out["emb"].shape[1]).astype(np.int64))
            dist = np.where((face_mask[:, None] & G.groups_table()[G.rows_of(names)][None, :]) != 0, dist, np.inf)
        return {"names": names, "dist_rows": dist}

    def _stream_quality(self, eng, frames_bgr, out) -> List[Dict[str, Any]]:
        """quality dicts of a fetched batch's faces, frame by frame (the order of the face dicts), from the frames still resident on `eng`"""
        frames = frames_bgr if isinstance(frames_bgr, _SOURCE_BATCHES) or frames_bgr.ndim == 4 else frames_bgr[None]
        H, W = frames_hw(frames)
        K = out["boxes"].shape[1]
        faces = [(b, box_to_location(out["boxes"][b, k], H, W)) for b, c in enumerate(out["counts"]) for k in range(min(int(c), K))]
        return self._quality_of(eng, frames, faces, rgb=False)

    def process_stream(self, batches, max_faces: int = 10, threshold: Optional[float] = None,
                       det_thresh: Optional[float] = None, all_matches: bool = False, quality: bool = False,
                       det_scales: Optional[Sequence[float]] = None, groups=None, streams=None):
        """process_frames for a stream of batches with TWO batches in flight on the GPU (lanes.py: a second handle and
        host thread; +7...13 % faces/s).  Yields one process_frames result per batch, in order.  Enrolment and deletion
        may run concurrently: they wait for the batches inside their device call and reach both gallery copies under
        the same lock, so every result is the one process_frames would have given for SOME gallery state between the
        batch's submission and its delivery.  Falls back to one lane when the second one cannot join (see _eng2).
        groups: as process_frames, for every batch - or a callable batch -> masks (mixer.run_mixed: the streams of each batch).
        streams: as process_frames, for every batch - or a callable batch -> streams (mixer.run_mixed(track=True)).  A tracked stream runs
        on ONE lane only: the track state lives in a handle, and alternate batches on a second handle would each see every other
        frame of a camera - every track would age twice as fast and neither handle could reuse what the other embedded."""
        engines = [self._eng()]
        e2 = self._eng2() if streams is None else None
        if e2 is not None:
            engines.append(e2)
        if streams is not None and not engine_caps(engines[0]).track:
            raise ValueError("streams needs an engine with face tracks (track_config)")
        for e in engines:
            _check_det_scales(engine_caps(e), det_scales)  # (here, not at the first batch)

        def on(eng):
            def run(frames, take_next=None, staged=None):
                return self._process_frames_on(eng, self.ENCODINGS.reading(), frames, max_faces, threshold, det_thresh, all_matches,
                                               take_next, staged, quality=quality, det_scales=det_scales,
                                               groups=groups(frames) if callable(groups) else groups,
                                               streams=streams(frames) if callable(streams) else streams)
            if not engine_caps(eng).lane:
                return lambda frames, take_next: run(frames)
            staged = {}                         # which batch sits in this lane's staging buffer

            def fn(frames, take_next):
                with eng.sequence():            # upload -> swap -> process -> fetch of one lane is one uninterrupted sequence
                    return run(frames, take_next, staged)
            return fn
        return lanes.run_ordered(batches, [on(e) for e in engines], prefetch=True)

    # ------------------------------------------------------------------ face tracks (process_frames / process_stream with streams=)
    def _track_engine(self):
        eng = self._eng()
        if not engine_caps(eng).track:
            raise ValueError("face tracks need an engine with track_config")
        return eng

    def configure_tracks(self, max_streams: int, iou_min: float = tracks.DEFAULT_IOU_MIN, refresh: int = tracks.DEFAULT_REFRESH,
                         max_missed: int = tracks.DEFAULT_MAX_MISSED) -> None:
        """face tracks for the passes that get streams=: up to max_streams (1..64) cameras; a detection continues a track when its IoU with
        the track's last box is at least iou_min, a track is embedded again every `refresh` frames and dropped after max_missed frames
        without a detection (tracks.TrackModel; the defaults are ordinary ones, not measured optima).  Clears every track.
        max_streams = 0 turns tracking off and frees its device memory.  The first lane's handle only: see process_stream."""
        if max_streams:
            tracks.check_config(iou_min, refresh, max_missed, max_streams)
        self._track_engine().track_config(max_streams, iou_min, refresh, max_missed)

    def reset_tracks(self, stream: Optional[int] = None) -> None:
        """forget the tracks of one stream (a camera that reconnected), None: of all"""
        self._track_engine().track_reset(-1 if stream is None else int(stream))

    def track_statistics(self) -> Dict[str, int]:
        """faces embedded and faces that reused their track's result, over the tracked passes since configure_tracks"""
        embedded, reused = self._track_engine().track_stats()
        return {"embedded": embedded, "reused": reused}

    def frame_buffer(self, batch: int, height: int, width: int) -> np.ndarray:
        """A page-locked u8 [batch, height, width, 3] array (owned by the engine, freed with it) for the capture / decode
        threads to write frames into.  process_frames / process_stream accept any array; one that lives in page-locked
        memory is copied to the GPU by DMA at PCIe rate, an ordinary (pageable) numpy array goes through the runtime's
        staging copies first - at 32 x 1080p (199 MB per batch) that is the difference between the engine's rate and
        ~0.8 of it (bench.py: config.service_api).  Reference: frames come out of cv2.VideoCapture.read() as fresh
        pageable arrays (routes/camera.py:204-209); a capture loop on this service reads into these buffers instead."""
        return self._eng().host_frames(batch, height, width)

    def process_frame(self, frame_bgr_or_path, metadata: Optional[Dict[str, Any]] = None):
        if isinstance(frame_bgr_or_path, str):
            frame = np.ascontiguousarray(load_image_file(frame_bgr_or_path)[..., ::-1])
        else:
            frame = frame_bgr_or_path
        cfg = metadata or {}
        return self.process_frames(frame[None], max_faces=int(cfg.get("max_faces", 10)),
                                   threshold=cfg.get("confidence_threshold"), det_scales=cfg.get("det_scales"))[0]

    # ------------------------------------------------------------------ statistics / housekeeping (:617-763)
    def get_quality_statistics(self) -> Dict[str, Any]:
        if not self._quality_history:
            return {"total_assessments": 0, "average_score": 0, "average_blur_score": 0, "average_lighting_score": 0}
        s = [q["score"] for q in self._quality_history]
        bl = [q["blur_score"] for q in self._quality_history]
        li = [q["lighting_score"] for q in self._quality_history]
        return {"total_assessments": len(s), "average_score": round(float(np.mean(s)), 2),
                "min_score": round(float(np.min(s)), 2), "max_score": round(float(np.max(s)), 2),
                "average_blur_score": round(float(np.mean(bl)), 2), "average_lighting_score": round(float(np.mean(li)), 2),
                "std_deviation": round(float(np.std(s)), 2)}

    def get_performance_metrics(self) -> Dict[str, Any]:
        with self._metrics_lock:
            m = dict(self._metrics)
        enc, cmp_ = m["total_encodings"], m["total_comparisons"]
        req = m["cache_hits"] + m["cache_misses"]
        attempts = enc + m["failed_encodings"]
        return {**m,
                "average_encoding_time": round(m["cumulative_encoding_time"] / enc, 4) if enc else 0.0,
                "average_comparison_time": round(m["cumulative_comparison_time"] / cmp_, 4) if cmp_ else 0.0,
                "cache_hit_rate": round(m["cache_hits"] / req * 100.0, 2) if req else 0.0,
                "encoding_success_rate": round(enc / attempts * 100.0, 2) if attempts else 100.0,
                "cache_size": len(self._encoding_cache), "total_faces_stored": len(self.ENCODINGS),
                "comparison_history_size": len(self._comparison_history)}

    def get_device_counters(self) -> Dict[str, Any]:
        """per-stage HIP-event times and algorithmic work from the native library (frp_get_counters)."""
        return self._eng().counters()

    def clear_cache(self) -> Dict[str, Any]:
        with self._cache_lock:
            n = len(self._encoding_cache)
            self._encoding_cache.clear()
        return {"success": True, "cleared_entries": n}

    def optimize_storage(self) -> Dict[str, Any]:
        cleaned = self._clean_cache()
        synced = 0
        for target in self.ENCODINGS.names():
            try:
                if not self._storage.has(target):
                    self._storage.store_embedding(target, self.ENCODINGS[target])
                    synced += 1
            except Exception as e:
                logger.debug("Sync failed for %s: %s", target, e)
        return {"success": True, "cache_entries_cleaned": cleaned, "database_synced": synced,
                "current_cache_size": len(self._encoding_cache), "total_faces": len(self.ENCODINGS)}

    def reset_metrics(self) -> Dict[str, Any]:
        with self._metrics_lock:
            old = dict(self._metrics)
            self._metrics = {k: (0.0 if k.startswith("cumulative") else 0) for k in _METRIC_KEYS}
        return {"success": True, "previous_metrics": old}

    def health_check(self) -> Dict[str, Any]:
        health = {"status": "healthy", "issues": [], "warnings": []}
        if len(self.ENCODINGS) == 0:
            health["warnings"].append("No faces enrolled in system")
        if len(self._encoding_cache) > 1000:
            health["warnings"].append(f"Large cache size: {len(self._encoding_cache)}")
        with self._metrics_lock:
            if self._metrics.get("failed_encodings", 0) > 100:
                health["warnings"].append(f"High failure rate: {self._metrics['failed_encodings']}")
        try:
            self._storage.ping()
        except Exception as db_err:
            health["status"] = "degraded"
            health["issues"].append(f"Database connectivity issue: {db_err}")
        if len(health["issues"]) > 2:
            health["status"] = "unhealthy"
        return health

    # ------------------------------------------------------------------ cache / backup helpers (:699-741)
    def _add_to_cache(self, key: str, data: Dict[str, Any]):
        with self._cache_lock:
            self._encoding_cache[key] = {"data": data, "timestamp": datetime.now()}

    def _get_from_cache(self, key: str) -> Optional[Dict[str, Any]]:
        with self._cache_lock:
            entry = self._encoding_cache.get(key)
            if not entry:
                return None
            if (datetime.now() - entry["timestamp"]).total_seconds() > self._cache_ttl:
                del self._encoding_cache[key]
                return None
            return entry["data"]

    def _remove_from_cache(self, key: str):
        with self._cache_lock:
            self._encoding_cache.pop(key, None)

    def _clean_cache(self) -> int:
        with self._cache_lock:
            now = datetime.now()
            dead = [k for k, v in self._encoding_cache.items() if (now - v["timestamp"]).total_seconds() > self._cache_ttl]
            for k in dead:
                del self._encoding_cache[k]
            return len(dead)

    def _backup_encoding_atomic(self, target_name: str, encoding: List[float]):
        BACKUP_DIR.mkdir(parents=True, exist_ok=True)
        final = BACKUP_DIR / f"{target_name}_backup.json"
        tmp = BACKUP_DIR / f"{target_name}_backup.json.tmp"
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump({"target": target_name, "encoding": encoding, "timestamp": datetime.now().isoformat(), "version": 1},
                      f, indent=2)
            f.flush()
            os.fsync(f.fileno())
        tmp.replace(final)


# Module singleton, as face_service.py:769.  The HIP engine behind it is created on first use.
face_service = FaceService()

# Module-level hooks probed by services/async_task_manager.py:125
process_frames = face_service.process_frames
process_frame = face_service.process_frame
process_image = face_service.process_frame
recognize = face_service.process_frame
search_face = face_service.find_k_nearest
find_matches = face_service.compare_faces
