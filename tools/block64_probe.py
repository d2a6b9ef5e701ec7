#!/usr/bin/env python3
"""The fused residual-block launch (conv3x3_block64.hip) against the two conv launches it replaces (each on the kernel the launcher
routes it to) on the headline workload's shapes (32 x 1080p frames, 320 faces) and a few smaller calls: same process, alternating,
best of 3; microseconds, the fused launch's algorithmic traffic (one read of x, one write of out) in GB/s, the plan's fill.
    python tools/block64_probe.py [iters]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lab  # noqa: E402,F401  (selects libfrp_lab.so)
import frp_amd_loader  # noqa: E402,F401
from frp_amd import native  # noqa: E402

BLOCK = 1 << 23
SHAPES = [  # name, N, H, W, conv1 act, conv1 flags, conv2 act, blocks per step
    ("det.layer1.0 32x272x480 ReLU / +x ReLU", 32, 272, 480, 1, 0, 1, 1),
    ("emb.layer1.1-2 320x56x56 PReLU border / +x", 320, 56, 56, 2, 1, 0, 2),
    ("det.layer1.0 4x272x480", 4, 272, 480, 1, 0, 1, 0),
    ("det.layer1.0 8x184x320 (720p)", 8, 184, 320, 1, 0, 1, 0),
    ("emb.layer1.x 128x56x56", 128, 56, 56, 2, 1, 0, 0),
    ("emb.layer1.x 37x56x56", 37, 56, 56, 2, 1, 0, 0),
]


def fill(N, H, W, ncu=256):
    """conv3x3_block64_plan's choice: (segments, steps, fill)"""
    strips, best = -(-W // 30), None
    for want in (1, 2, 4, 8):
        rows = (-(-H // want) + 3) // 4 * 4
        if want > 1 and rows < 8:
            break
        segs, steps = -(-H // rows), (min(rows, H) + 2 + 3) // 4 + 1
        rounds = -(-N * strips * segs // ncu)
        if best is None or rounds * steps < best[0]:
            best = (rounds * steps, segs, steps, N * H * W / (rounds * ncu * steps * 120.0))
    return best[1:]


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    eng = native.Engine(0)
    tot = [0.0, 0.0]
    for name, N, H, W, act1, fl1, act2, cnt in SHAPES:
        best = [1e30, 1e30, 1e30]
        for _ in range(3):
            best[0] = min(best[0], eng.conv_bench(N, H, W, 64, 64, 3, 1, act1, fl1, False, iters) * 1e3)
            best[1] = min(best[1], eng.conv_bench(N, H, W, 64, 64, 3, 1, act2, 0, True, iters) * 1e3)
            best[2] = min(best[2], eng.conv_bench(N, H, W, 64, 64, 3, 1, act1, fl1 | BLOCK, False, iters) * 1e3)
        two = best[0] + best[1]
        tot[0] += two * cnt
        tot[1] += best[2] * cnt
        segs, steps, f = fill(N, H, W)
        print(f"{name:44s} conv1 {best[0]:7.1f} + conv2 {best[1]:7.1f} = {two:7.1f} us | fused {best[2]:7.1f} us {N * H * W * 256 / best[2] / 1e3:7.1f} GB/s "
              f"x{two / best[2]:.3f} | segs {segs} steps {steps} fill {f:.3f}", flush=True)
    print(f"per step (blocks per step applied): two launches {tot[0]:.1f} us, fused {tot[1]:.1f} us")


if __name__ == "__main__":
    main()
