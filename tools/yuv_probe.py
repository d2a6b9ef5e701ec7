#!/usr/bin/env python3
"""YUV 4:2:0 ingest against raw BGR ingest: how long until a batch of 1080p frames is resident, by route.  One process, the routes
alternating batch by batch, warmed, every source in page-locked memory; per route the wall time of the staged upload + swap_frames +
synchronise over `batches` batches, repeated `repeats` times: the mean of every repeat, their spread, per-batch extremes.
    (a) upload_frames_async, BGR (3 bytes per pixel over PCIe): the existing path, the baseline
    (b) upload_yuv_async, NV12 from the host (1.5 bytes per pixel), one pool of surfaces
    (c) upload_yuv_async, I420 from the host, three planes per frame
    (d) upload_yuv_async, NV12 surfaces that already lie in device memory (pitch 2048): the table copy and the kernel
    python3 tools/yuv_probe.py [B] [batches] [repeats]
The kernel alone - against its byte bound, (1.5 + 3) bytes per pixel at the 4.5 TB/s DESIGN.md uses -: one run of its own under
    rocprofv3 --kernel-trace --stats -d out -o kt -- python3 tools/yuv_probe.py 32 6 1"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: E402  (before the engine: one HIP runtime in the process)
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native, yuv  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
R = int(sys.argv[3]) if len(sys.argv) > 3 else 3
H, W = 1080, 1920
eng = native.Engine(0, max_batch=B, max_faces=10, max_h=H, max_w=W)
bgr = eng.host_frames(B, H, W)
bgr[:] = bench.synth_frames(B, H, W, 10, 77)
# full-range YCbCr of those frames, chroma averaged over 2 x 2 (any plausible content does: the kernel's time does not depend on it)
f = bgr.astype(np.float32)
y = 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]
sub = lambda c: c.reshape(B, H // 2, 2, W // 2, 2).mean((2, 4))      # noqa: E731
q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)            # noqa: E731
Y, U, V = q(y), q(128 + 0.564 * sub(f[..., 0] - y)), q(128 + 0.713 * sub(f[..., 2] - y))
nv12 = eng.host_frames(B, H // 2, W).reshape(B, H * 3 // 2, W)       # page-locked, B x (H * 3 / 2) rows of W bytes
nv12[:, :H] = Y
nv12[:, H:, 0::2], nv12[:, H:, 1::2] = U, V
i420 = eng.host_frames(B, H // 2, W).reshape(B, H * W * 3 // 2)
i420[:, :H * W] = Y.reshape(B, -1)
i420[:, H * W:H * W * 5 // 4] = U.reshape(B, -1)
i420[:, H * W * 5 // 4:] = V.reshape(B, -1)
b_nv12 = yuv.YuvBatch([yuv.YuvFrame(nv12[b, :H], nv12[b, H:]) for b in range(B)], "NV12", "JFIF")
b_i420 = yuv.YuvBatch([yuv.YuvFrame(i420[b, :H * W].reshape(H, W), i420[b, H * W:H * W * 5 // 4].reshape(H // 2, W // 2),
                                    i420[b, H * W * 5 // 4:].reshape(H // 2, W // 2)) for b in range(B)], "I420", "JFIF")
PITCH, ROWS = 2048, 1088 + 544                                         # a decoder's pool: pitch and plane heights rounded up
pool = torch.zeros((B, ROWS, PITCH), dtype=torch.uint8, device="cuda:0")
pool[:, :H, :W] = torch.from_numpy(np.ascontiguousarray(nv12[:, :H]))
pool[:, 1088:1088 + H // 2, :W] = torch.from_numpy(np.ascontiguousarray(nv12[:, H:]))
torch.cuda.synchronize()
base = pool.data_ptr()
b_dev = yuv.YuvBatch([yuv.YuvFrame(base + b * ROWS * PITCH, base + (b * ROWS + 1088) * PITCH, device=True, hw=(H, W), y_pitch=PITCH, c_pitch=PITCH)
                      for b in range(B)], "NV12", "JFIF")
ROUTES = [("(a) BGR host, upload_frames_async", lambda: eng.upload_frames_async(bgr), 3.0),
          ("(b) NV12 host, upload_yuv_async", lambda: eng.upload_yuv_async(b_nv12), 1.5),
          ("(c) I420 host, upload_yuv_async", lambda: eng.upload_yuv_async(b_i420), 1.5),
          ("(d) NV12 device, upload_yuv_async", lambda: eng.upload_yuv_async(b_dev), 0.0)]


def one(stage):
    t0 = time.perf_counter()
    stage()
    t1 = time.perf_counter()
    eng.swap_frames()
    eng.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


# the four routes end with the same frames (to the conversion: (a) holds the BGR source, the others its YCbCr round trip)
want = yuv.to_bgr(nv12[:2, :H], nv12[:2, H:], layout="NV12", matrix="JFIF")
for name, stage, _ in ROUTES[1:]:
    one(stage)
    assert np.array_equal(eng.get_frames(0, 2), want), name
for _, stage, _ in ROUTES:              # warm: buffers, code objects
    for _ in range(3):
        one(stage)
res = {name: [] for name, _, _ in ROUTES}
for r in range(R):
    acc = {name: [] for name, _, _ in ROUTES}
    for _ in range(N):
        for name, stage, _ in ROUTES:   # alternating: drift of the box hits every route alike
            acc[name].append(one(stage))
    for name in acc:
        res[name].append(np.array(acc[name]))
px = B * H * W
print(f"{B} x {H} x {W} frames, page-locked sources; {R} repeats of {N} batches, routes alternating")
print(f"kernel byte bound: {px * 4.5 / 1e6:.0f} MB at 4.5 TB/s = {px * 4.5 / 4.5e12 * 1e6:.0f} us")
for name, _, bpp in ROUTES:
    rep = [a[:, 1].mean() for a in res[name]]
    allb = np.concatenate([a[:, 1] for a in res[name]])
    call = np.concatenate([a[:, 0] for a in res[name]]).mean()
    mean = float(np.mean(rep))
    rate = f"; {px * bpp / mean / 1e6:.1f} GB/s over PCIe" if bpp else ""
    print(f"{name:36s} resident after {mean:6.2f} ms (repeats: {', '.join(f'{x:.2f}' for x in rep)}; spread of repeats {max(rep) - min(rep):.2f}; "
          f"per batch min {allb.min():.2f} max {allb.max():.2f} std {allb.std():.2f}); call returned after {call:.2f} ms{rate}")
eng.close()
