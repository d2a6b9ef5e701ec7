#!/usr/bin/env python3
"""Face quality: frp_face_quality on resident frames against the host method (FaceService.assess_face_quality) over the same crops -
(a) 32 x 1080p resident, 10 boxes per frame (one call, 320 rectangles), (b) one 4K frame, the whole frame as the crop.
Per case: the device call (a host clock around Engine.face_quality, which uploads the rectangles, runs both kernels, copies the sums
and waits: best of 20), the bytes of the crops over the achievable HBM rate (6.3 TB/s: the kernel's lower bound), and the host
method on one thread and on 16.  The kernels' own time comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d out -o kt -- python3 tools/quality_probe.py
(face_quality_kernel, face_quality_reduce_kernel: 21 calls of each per case).  The dicts of both paths are compared on the way.
    python tools/quality_probe.py"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native  # noqa: E402
from frp_amd.face_service import FaceService  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
THREADS = 16


def boxes(rng, B, H, W, per_frame):
    """face-sized rectangles (frame, top, right, bottom, left): 1/6 ... 1/2 of the frame's height, anywhere"""
    r = []
    for b in range(B):
        for _ in range(per_frame):
            h = int(rng.integers(H // 6, H // 2))
            w = int(h * rng.uniform(0.7, 1.0))
            top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            r.append((b, top, left + w, top + h, left))
    return r


def case(eng, name, frames, rects):
    B, H, W, _ = frames.shape
    eng.upload_frames(frames)
    sums = eng.face_quality(rects)
    best = 1e9
    for _ in range(20):
        t0 = time.perf_counter()
        eng.face_quality(rects)
        best = min(best, time.perf_counter() - t0)
    nbytes = sum((r[3] - r[1]) * (r[2] - r[4]) * 3 for r in rects)
    fs = FaceService(engine=eng)
    dev = [fs.quality_from_sums((H, W, 3), r[1:], (r[3] - r[1]) * (r[2] - r[4]), s) for r, s in zip(rects, sums)]
    rgb_views = [f[..., ::-1] for f in frames]                     # the frames are BGR: the host method takes RGB
    one = lambda r: fs.assess_face_quality(rgb_views[r[0]], r[1:])
    t0 = time.perf_counter()
    host = [one(r) for r in rects]
    t_host1 = time.perf_counter() - t0
    with ThreadPoolExecutor(THREADS) as ex:
        t0 = time.perf_counter()
        host_t = list(ex.map(one, rects))
        t_hostn = time.perf_counter() - t0
    assert dev == host == host_t, "device and host quality differ"
    print(f"{name}: {len(rects)} rectangles, {nbytes / 1e6:.1f} MB of crop pixels")
    print(f"  device call (rectangles up, 2 kernels, sums down, wait)   {best * 1e3:9.3f} ms")
    print(f"  crop bytes / {HBM_BYTES_PER_S / 1e12:.1f} TB/s (lower bound of the kernel)        {nbytes / HBM_BYTES_PER_S * 1e3:9.3f} ms")
    print(f"  host method, one thread                                   {t_host1 * 1e3:9.1f} ms")
    print(f"  host method, {THREADS} threads ({len(os.sched_getaffinity(0))} available)                     {t_hostn * 1e3:9.1f} ms")


def main():
    rng = np.random.default_rng(5)
    eng = native.Engine(0, max_batch=32, max_faces=10, max_h=2160, max_w=3840)
    frames = bench.synth_frames(32, 1080, 1920, 10, 77)
    case(eng, "32 x 1080p, 10 boxes per frame", frames, boxes(rng, 32, 1080, 1920, 10))
    still = np.ascontiguousarray(np.tile(frames[:1], (1, 2, 2, 1)))
    case(eng, "one 4K frame, whole-frame crop", still, [(0, 0, 3840, 2160, 0)])
    eng.close()


if __name__ == "__main__":
    main()
