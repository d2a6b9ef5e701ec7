#!/usr/bin/env python3
"""JPEG encode: frp_encode_jpeg on resident frames against the only route there was before it - the raw frames fetched to the host
(frp_get_det_source: 6.2 MB per 1080p frame over PCIe) and PIL / libjpeg on 16 threads -
(a) 32 x 1080p resident frames, whole frames, (b) 320 face crops of 160 x 160 out of them; quality 95, 4:2:0, no restart intervals.
Per case: the device call (a host clock around Engine.encode_jpeg's library call, which uploads the rectangles, runs the forward and
entropy kernels with two size read-backs, copies the files and waits: best of 10), the bytes returned, the pixel and coefficient
bytes the kernels move over the achievable HBM rate (6.3 TB/s: their lower bound), and the host route.  The files of both routes are
compared on the way.  Three routes side by side for the optimised Huffman tables (FRP_FLAG_JPEG_OPTIMIZE: a histogram kernel, one more
read-back and wait, table generation on the host): the device call without and with the flag - timed alternately in the same loop,
best and median of 10 each - the bytes each returns, and the host route with save(optimize=True).  The kernels' own times come from a
run of its own:
    rocprofv3 --kernel-trace --stats -d out -o kt -- python3 tools/jpeg_encode_probe.py
    python tools/jpeg_encode_probe.py"""
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
THREADS = 16
QUALITY = 95


def pil_jpeg(rgb, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=QUALITY, subsampling=2, optimize=optimize)
    return buf.getvalue()


def pil_jpeg_optimized(rgb):
    return pil_jpeg(rgb, True)


def case(eng, name, frames, rects):
    eng.upload_frames(frames)
    files = eng.encode_jpeg(rects, quality=QUALITY)
    files_opt = eng.encode_jpeg(rects, quality=QUALITY, optimize=True)
    times = {False: [], True: []}
    for _ in range(10):                                           # the two device routes alternate: the same box, the same minute
        for optimize in (False, True):
            t0 = time.perf_counter()
            eng.encode_jpeg(rects, quality=QUALITY, optimize=optimize)
            times[optimize].append(time.perf_counter() - t0)
    best, best_opt = min(times[False]), min(times[True])
    med, med_opt = statistics.median(times[False]), statistics.median(times[True])
    px = sum((r[3] - r[1]) * (r[2] - r[4]) for r in rects)
    blocks = sum(-(-(r[3] - r[1]) // 16) * -(-(r[2] - r[4]) // 16) * 6 for r in rects)
    out_bytes = sum(map(len, files))
    # forward: the pixels once (chroma reads them again out of cache), coefficients written; entropy: coefficients read twice
    # (bits, pack), the stream written (atomics), read twice (0xFF counts, emit) and written once more as stuffed bytes
    traffic = px * 3 + blocks * 128 * 3 + out_bytes * 4
    with ThreadPoolExecutor(THREADS) as ex:
        t0 = time.perf_counter()
        host = eng.det_source()                                   # the parent's route: raw frames over PCIe ...
        t_fetch = time.perf_counter() - t0
        crops = [np.ascontiguousarray(host[r[0], r[1]:r[3], r[4]:r[2], ::-1]) for r in rects]
        t0 = time.perf_counter()
        ref = list(ex.map(pil_jpeg, crops))                      # ... and libjpeg on the host
        t_pil = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref_opt = list(ex.map(pil_jpeg_optimized, crops))        # ... with optimize=True: libjpeg's two passes
        t_pil_opt = time.perf_counter() - t0
    assert ref == files, "device and PIL files differ"
    assert ref_opt == files_opt, "device and PIL files differ with optimised tables"
    out_opt = sum(map(len, files_opt))
    print(f"{name}: {len(rects)} files, {px * 3 / 1e6:.1f} MB of pixels -> {out_bytes / 1e6:.2f} MB of JPEG ({out_bytes / len(rects) / 1e3:.1f} kB per file)")
    print(f"  device call (rectangles up, kernels, 2 size read-backs, files down, wait)  {best * 1e3:9.3f} ms")
    print(f"  bytes returned over PCIe                                                    {out_bytes / 1e6:9.2f} MB")
    print(f"  kernel traffic {traffic / 1e6:.0f} MB / {HBM_BYTES_PER_S / 1e12:.1f} TB/s (lower bound of the kernels)              {traffic / HBM_BYTES_PER_S * 1e3:9.3f} ms")
    print(f"  host route: raw frames fetched ({host.nbytes / 1e6:.1f} MB)                              {t_fetch * 1e3:9.1f} ms")
    print(f"  host route: PIL encode, {THREADS} threads ({len(os.sched_getaffinity(0))} available)                          {t_pil * 1e3:9.1f} ms")
    print(f"  optimised tables, same loop: device call without the flag  best {best * 1e3:9.3f} ms  median {med * 1e3:9.3f} ms  {out_bytes / 1e6:9.2f} MB returned")
    print(f"                               device call with the flag     best {best_opt * 1e3:9.3f} ms  median {med_opt * 1e3:9.3f} ms  {out_opt / 1e6:9.2f} MB returned"
          f"  ({(best_opt / best - 1) * 100:+.1f} % time, {(out_opt / out_bytes - 1) * 100:+.1f} % bytes)")
    print(f"                               host route: PIL save(optimize=True), {THREADS} threads                 {t_pil_opt * 1e3:9.1f} ms")


def main():
    rng = np.random.default_rng(6)
    eng = native.Engine(0, max_batch=32, max_faces=10, max_h=1080, max_w=1920)
    frames = bench.synth_frames(32, 1080, 1920, 10, 77)
    case(eng, "32 x 1080p, whole frames", frames, [(b, 0, 1920, 1080, 0) for b in range(32)])
    crops = []
    for i in range(320):
        top, left = int(rng.integers(0, 1080 - 160 + 1)), int(rng.integers(0, 1920 - 160 + 1))
        crops.append((i % 32, top, left + 160, top + 160, left))
    case(eng, "320 face crops of 160 x 160", frames, crops)
    eng.close()


if __name__ == "__main__":
    main()
