#!/usr/bin/env python3
"""BASELINE config 4 as one device pass against the host route: ms per step of both, one handle, one process.
4 x 2160 x 3840 resident frames, scales (1, .5, .25), the score threshold calibrated as bench.py:run_config4 calibrates it,
galleries of 100 k and 1 M rows.  The two routes alternate round by round (`rounds` rounds of `steps` steps each, after a
warm-up round of both); per route the mean of its rounds, and the round-to-round spread (max - min) of the host route -
the bar: the device route is no slower than the host route by more than that spread.
    host route    detect_resident per scale (blocking) + pyramid.merge_scales + finish_faces: bench.py's config-4 step
    device route  process_pyramid_resident + fetch_results
Also: whether the device route replays from the graph cache (frp_debug_graph_replays around one warmed call), with three
scales and with a fourth.
    python3 tools/pyramid_probe.py [rounds] [steps] [gallery rows ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native, pyramid, weights  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
GALLERIES = [int(a) for a in sys.argv[3:]] or [100_000, 1_000_000]
B, K, H, W = 4, 10, 2160, 3840
SCALES = (1.0, 0.5, 0.25)
HWS = [pyramid.scaled_size(H, W, s) for s in SCALES]

eng = native.Engine(0, max_batch=B, max_faces=K, max_h=H, max_w=W)
eng.load_weights(weights.pack_blob(weights.make_synthetic_raw(7)))
eng.upload_frames(bench.synth_frames(B, H, W, K, 4321))
probe = eng.detect_resident((H, W), max_faces=64, det_thresh=1e-6, nms_iou=0.4)
kth = np.sort(probe["scores"], axis=1)[:, ::-1][:, K - 1]
thr = float(np.clip(np.median(kth[kth > 0]) if np.any(kth > 0) else 0.5, 1e-4, 0.9999))
print(f"B={B} K={K} {H}x{W} scales={SCALES} det_thresh={thr:.6f} rounds={ROUNDS} steps={STEPS}", flush=True)


def host_step():
    per = [(hw, eng.detect_resident(hw, max_faces=64, det_thresh=thr, nms_iou=0.4)) for hw in HWS]
    boxes, kps, scores, counts = pyramid.merge_scales(per, (H, W), K, 0.4)
    return eng.finish_faces(boxes, kps, scores, counts, K)


def device_step(hws=HWS):
    eng.process_pyramid_resident(hws, per_scale=64, max_faces=K, det_thresh=thr, nms_iou=0.4)
    return eng.fetch_results()


def timed(step):
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    eng.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


for rows in GALLERIES:
    eng.gallery_set(bench.gallery_rows(rows, 0, rows))
    a, b = host_step(), device_step()
    same = all(np.array_equal(a[k], b[k]) for k in ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos"))
    timed(host_step), timed(device_step)                       # warm-up round of both
    host, dev = [], []
    for _ in range(ROUNDS):
        host.append(timed(host_step))
        dev.append(timed(device_step))
    spread = max(host) - min(host)
    print(f"gallery {rows}: faces/step {int(a['counts'].sum())}, routes bit-identical: {same}")
    print(f"  host route   ms/step mean {np.mean(host):.3f}  rounds {' '.join(f'{v:.3f}' for v in host)}  spread {spread:.3f}")
    print(f"  device route ms/step mean {np.mean(dev):.3f}  rounds {' '.join(f'{v:.3f}' for v in dev)}  spread {max(dev) - min(dev):.3f}")
    print(f"  device - host {np.mean(dev) - np.mean(host):+.3f} ms/step; bar (no slower than the host route by more than its spread): "
          f"{'met' if np.mean(dev) <= np.mean(host) + spread else 'MISSED'}", flush=True)

# graph cache: network passes replayed from a captured graph by ONE warmed device-route call (3 detector shapes + the embedder)
for hws, name in ((HWS, "3 scales"), (HWS + [pyramid.scaled_size(H, W, 0.75)], "4 scales")):
    for _ in range(3):
        device_step(hws)
    r0 = eng.graph_replays()
    device_step(hws)
    print(f"graph replays in one warmed call, {name}: {eng.graph_replays() - r0} of {len(hws) + 1} network passes", flush=True)
eng.close()
