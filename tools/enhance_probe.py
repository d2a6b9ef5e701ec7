#!/usr/bin/env python3
"""Snapshot enhancer: Engine.encode_jpeg_enhanced on resident frames against the route it replaces - the raw frame fetched to the host
(frp_get_frames: 6.2 MB per 1080p frame over PCIe), Pillow's resize(BICUBIC) + UnsharpMask(1, 120, 3) and Pillow's JPEG encoder at
quality 85, on one thread, as services/enhancer.py runs them -
(a) one 1080p frame -> 2667 x 1500 (enhanced_size at the reference's defaults), (b) 32 face crops of 160 x 160 -> 320 x 320.
Per case, after a warm-up of both routes: the device call (a host clock around the library call, which uploads rectangles and tap
tables, runs the enhance kernel and the encoder with its two size read-backs, copies the files and waits) and the host route, each
repeated until half a second has passed and at least 10 times, median and best; the pixel call (frp_enhance_pixels) alone, which
returns out_w * out_h * 3 bytes over PCIe; the bytes the enhance kernel moves over the achievable HBM rate (its lower bound).  The
files of both routes are compared on the way.  Three routes side by side for the optimised Huffman tables (optimize=True: the file the
reference writes): the device call without and with the flag, the bytes each returns, and the host route with save(optimize=True).
The kernels' own times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d out -o kt -- python3 tools/enhance_probe.py
    python tools/enhance_probe.py"""
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native  # noqa: E402
from frp_amd.face_service import enhanced_size  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
QUALITY = 85


def timed(fn, min_seconds=0.5, min_runs=10):
    times, t_end = [], time.perf_counter() + min_seconds
    while len(times) < min_runs or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), len(times)


def host_route(eng, rects, sizes, optimize=False):
    """what the feature replaces: the frames over PCIe, then Pillow on this thread"""
    from PIL import Image, ImageFilter
    frames = eng.get_frames()
    out = []
    for (b, top, right, bottom, left), size in zip(rects, sizes):
        im = Image.fromarray(np.ascontiguousarray(frames[b, top:bottom, left:right, ::-1]))
        if size != im.size:
            im = im.resize(size, Image.BICUBIC)
        im = im.filter(ImageFilter.UnsharpMask(radius=1, percent=120, threshold=3))
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=QUALITY, optimize=optimize)
        out.append(buf.getvalue())
    return out


def case(eng, name, frames, rects, sizes):
    eng.upload_frames(frames)
    files = eng.encode_jpeg_enhanced(rects, sizes, quality=QUALITY)          # warm-up of both routes, and the comparison
    assert host_route(eng, rects, sizes) == files, "device and Pillow files differ"
    files_opt = eng.encode_jpeg_enhanced(rects, sizes, quality=QUALITY, optimize=True)
    assert host_route(eng, rects, sizes, optimize=True) == files_opt, "device and Pillow files differ with optimised tables"
    dev = timed(lambda: eng.encode_jpeg_enhanced(rects, sizes, quality=QUALITY))
    dev_opt = timed(lambda: eng.encode_jpeg_enhanced(rects, sizes, quality=QUALITY, optimize=True))
    dev_again = timed(lambda: eng.encode_jpeg_enhanced(rects, sizes, quality=QUALITY))       # the spread of the route the flag is held against
    host_opt = timed(lambda: host_route(eng, rects, sizes, optimize=True))
    pix = timed(lambda: eng.enhance_pixels(rects, sizes))
    host = timed(lambda: host_route(eng, rects, sizes))
    fetch = timed(eng.get_frames)
    src_px = sum((r[3] - r[1]) * (r[2] - r[4]) for r in rects)
    out_px = sum(w * h for w, h in sizes)
    out_bytes = sum(map(len, files))
    traffic = 3 * (src_px + out_px)            # compulsory: every source pixel once, every output pixel once (halos come out of L2)
    print(f"{name}: {len(rects)} images, {src_px * 3 / 1e6:.2f} MB of pixels -> {out_px * 3 / 1e6:.2f} MB enhanced -> {out_bytes / 1e6:.2f} MB of JPEG")
    for label, (med, best, runs) in (("device: encode_jpeg_enhanced (tables up, enhance + encoder kernels, files down, wait)", dev),
                                     ("device: encode_jpeg_enhanced(optimize=True) (+ histogram kernel, counts down, tables up, one more wait)", dev_opt),
                                     ("device: encode_jpeg_enhanced without the flag, again", dev_again),
                                     ("host route with save(optimize=True), one thread", host_opt),
                                     ("device: enhance_pixels alone (tables up, enhance kernel, pixels down, wait)", pix),
                                     ("host route: get_frames + Pillow resize + UnsharpMask + save, one thread", host),
                                     ("  of which get_frames (all resident frames over PCIe)", fetch)):
        print(f"  {label:98s} median {med * 1e3:9.3f} ms  best {best * 1e3:9.3f} ms  ({runs} runs)")
    out_opt = sum(map(len, files_opt))
    print(f"  bytes returned: {out_bytes / 1e6:.3f} MB without the flag, {out_opt / 1e6:.3f} MB with it ({(out_opt / out_bytes - 1) * 100:+.1f} %)")
    print(f"  enhance kernel traffic {traffic / 1e6:.1f} MB / {HBM_BYTES_PER_S / 1e12:.1f} TB/s (lower bound of the kernel) {traffic / HBM_BYTES_PER_S * 1e3:9.4f} ms")


def main():
    rng = np.random.default_rng(6)
    eng = native.Engine(0, max_batch=32, max_faces=10, max_h=1080, max_w=1920)
    one = bench.synth_frames(1, 1080, 1920, 10, 77)
    size = enhanced_size(1920, 1080)
    assert size == (2667, 1500)
    case(eng, "one 1080p frame -> 2667 x 1500", one, [(0, 0, 1920, 1080, 0)], [size])
    frames = bench.synth_frames(4, 1080, 1920, 10, 78)
    crops = []
    for i in range(32):
        top, left = int(rng.integers(0, 1080 - 160 + 1)), int(rng.integers(0, 1920 - 160 + 1))
        crops.append((i % 4, top, left + 160, top + 160, left))
    case(eng, "32 face crops of 160 x 160 -> 320 x 320", frames, crops, [(320, 320)] * 32)
    eng.close()


if __name__ == "__main__":
    main()
