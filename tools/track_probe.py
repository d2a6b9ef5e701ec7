#!/usr/bin/env python3
"""What face tracks cost and what they can save, at the headline shape: 32 x 1080p resident frames, K = 10, 100 k gallery rows, the
full-depth synthetic blob, threshold mode (the threshold calibrated as bench.py calibrates it), one handle, one process.
ms per step of process_resident + fetch_results for
    (a) untracked          the parent path
    (b) tracked, refresh 1 every face is embedded in every step: (b) - (a) is what the tracker's four launches, the per-slot result
                           arrays and their fetch cost
    (c) tracked, refresh 8 on unchanged frames, one stream per frame: a face is embedded in one step of eight - an upper bound for a
                           static scene, not a claim about real video
The three alternate round by round (`rounds` rounds of `steps` steps each, after a warm-up round of all); per mode the mean of its
rounds and their spread (max - min).  The tracker's kernel durations come from a run of their own:
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/track_probe.py 1 16
The seeded detector head predicts negative left + right or top + bottom distances for about two faces of three: boxes with x2 < x1
or y2 < y1, which are empty under the +1-pixel IoU and continue no track.  The probe therefore replaces the head's four distance rows
by the constant 1.5 strides (weights 0, bias 1.5): the same logits, so the same anchors pass the threshold, and every box is 3 x 3
strides around its anchor.  All three modes run on that blob.
    python3 tools/track_probe.py [rounds] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa: E402,F401
import bench  # noqa: E402
from frp_amd import native, netspec, weights  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
B, K, H, W, ROWS = 32, 10, 1080, 1920, 100_000

eng = native.Engine(0, max_batch=B, max_faces=K, max_h=H, max_w=W)
raw = dict(weights.make_synthetic_raw(7))
frames = bench.synth_frames(B, H, W, K, 1234)
for lv in (3, 4, 5):
    w, b = raw[f"det.head{lv}.out.weight"].copy(), raw[f"det.head{lv}.out.bias"].copy()
    for anchor in range(2):
        rows = slice(anchor * netspec.DET_VALUES_PER_ANCHOR + 1, anchor * netspec.DET_VALUES_PER_ANCHOR + 5)      # left, top, right, bottom
        w[rows], b[rows] = 0.0, 1.5
    raw[f"det.head{lv}.out.weight"], raw[f"det.head{lv}.out.bias"] = w, b
eng.load_weights(weights.pack_blob(raw))
probe = eng.detect(frames, max_faces=64, det_thresh=1e-6, nms_iou=0.4)
kth = np.sort(probe["scores"], axis=1)[:, ::-1][:, K - 1]
thr = float(np.clip(np.median(kth[kth > 0]) if np.any(kth > 0) else 0.5, 1e-4, 0.9999))
eng.gallery_set(bench.gallery_rows(ROWS, 0, ROWS))
eng.upload_frames(frames)
print(f"B={B} K={K} {H}x{W} gallery={ROWS} det_thresh={thr:.6f} rounds={ROUNDS} steps={STEPS}", flush=True)


def step(flags):
    eng.process_resident(K, det_thresh=thr, nms_iou=0.4, flags=flags)
    return eng.fetch_results()


def timed(flags, refresh=None):
    if refresh is not None:                    # a new configuration clears the tracks: the first step embeds everything, outside the window
        eng.track_config(B, 0.3, refresh, 2)
        eng.set_frame_streams(np.arange(B))
        step(flags)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step(flags)
    eng.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


MODES = (("a untracked", 0, None), ("b tracked refresh=1", native.FLAG_TRACK, 1), ("c tracked refresh=8", native.FLAG_TRACK, 8))
want = step(0)
for name, flags, refresh in MODES[1:]:
    timed(flags, refresh)
    got = step(flags)
    same = all(np.array_equal(got[k], want[k]) for k in want)
    e, r = eng.track_stats()
    print(f"{name}: results bit-identical to the untracked pass: {same}; embedded {e} reused {r} over {STEPS + 2} steps", flush=True)
timed(0)
ms = {name: [] for name, _, _ in MODES}
for _ in range(ROUNDS):
    for name, flags, refresh in MODES:
        ms[name].append(timed(flags, refresh))
print(f"faces/step {int(want['counts'].sum())} (min {int(want['counts'].min())} max {int(want['counts'].max())} per frame)")
for name, v in ms.items():
    print(f"  {name:22s} ms/step mean {np.mean(v):.3f}  rounds {' '.join(f'{x:.3f}' for x in v)}  spread {max(v) - min(v):.3f}")
a, b, c = (np.mean(ms[name]) for name, _, _ in MODES)
print(f"  (b) - (a) {b - a:+.3f} ms/step (the feature's overhead); (c) - (a) {c - a:+.3f} ms/step; spread of (a) {max(ms[MODES[0][0]]) - min(ms[MODES[0][0]]):.3f}",
      flush=True)
eng.close()
