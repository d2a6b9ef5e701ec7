#!/usr/bin/env python3
"""JPEG ingest without restart markers: the host entropy decoder (the default) against the self-synchronising device decoder
(Engine.set_jpeg_selfsync) at several subsequence sizes.  Same build, same process, alternating, warmed; per setting the time from
upload_jpeg_async to the batch being resident (the call + swap + synchronise) over `batches` batches, repeated `repeats` times: mean of
every repeat, their spread, and the synchronisation rounds of the batch.
    python3 tools/jpeg_selfsync_probe.py [B] [quality] [batches] [repeats]
    rocprofv3 --kernel-trace --stats -d out -o kt -- python3 tools/jpeg_selfsync_probe.py 32 90 6 1 128        (one setting: per-kernel times)"""
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from PIL import Image
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 90
N = int(sys.argv[3]) if len(sys.argv) > 3 else 20
R = int(sys.argv[4]) if len(sys.argv) > 4 else 3
SETTINGS = [int(a) for a in sys.argv[5:]] or [0, 64, 128, 256]          # 0: the host decoder
frames = bench.synth_frames(B, 1080, 1920, 10, 77)
jpegs = []
for f in frames:
    b = io.BytesIO()
    Image.fromarray(f[..., ::-1]).save(b, "JPEG", quality=Q)
    jpegs.append(b.getvalue())
assert native.jpeg_info(jpegs[0])["restart_interval"] == 0
print(f"{B} x 1080p JPEG stills, quality {Q}, 4:2:0, no restart markers: {sum(map(len, jpegs)) / B / 1e3:.0f} kB each")
eng = native.Engine(0, max_batch=B, max_faces=10, max_h=1080, max_w=1920)


def one(setting):
    eng.set_jpeg_selfsync(setting)
    t0 = time.perf_counter()
    eng.upload_jpeg_async(jpegs)
    t1 = time.perf_counter()
    eng.swap_frames()
    eng.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


for s in SETTINGS:                      # warm: buffers, page-locked blocks, code objects
    for _ in range(3):
        one(s)
for s in SETTINGS:
    if s:
        _, st = eng.jpeg_selfsync_coefficients(jpegs, s)
        print(f"S = {s}: subsequences per image {int(st[:, 0].min())} .. {int(st[:, 0].max())}, synchronisation rounds {int(st[:, 1].min())} .. {int(st[:, 1].max())}")
res = {s: [] for s in SETTINGS}
for r in range(R):
    acc = {s: [] for s in SETTINGS}
    for _ in range(N):
        for s in SETTINGS:              # alternating: drift of the box hits every setting alike
            acc[s].append(one(s))
    for s in SETTINGS:
        res[s].append(np.array(acc[s]))
for s in SETTINGS:
    means = [a[:, 1].mean() for a in res[s]]
    allr = np.concatenate(res[s])
    name = "host decoder (setting off)" if s == 0 else f"self-sync, S = {s}"
    print(f"{name:28s} resident after {np.mean(means):7.2f} ms (repeats: {', '.join(f'{m:.2f}' for m in means)}; spread of repeats {max(means) - min(means):.2f}; "
          f"per batch min {allr[:, 1].min():.2f} max {allr[:, 1].max():.2f} std {allr[:, 1].std():.2f}); call returned after {allr[:, 0].mean():.2f} ms")
print("self-sync batches:", eng.jpeg_selfsync_batches(), " restart-interval device batches:", eng.jpeg_device_batches())
