"""Writes tests/golden/jpeg_encode/*.npz: input pixels (RGB u8) and the file PIL / libjpeg writes for them with restart intervals
(Image.save(..., restart_marker_blocks=r)), so that the GPU suite does not depend on its box's Pillow knowing that keyword.
    python tests/golden/make_jpeg_encode_golden.py
Each file: rgb [H, W, 3], jpeg (the bytes), quality, restart_mcus, subsampling ("4:2:0" / "4:4:4")."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_encode_model as M  # noqa: E402

CASES = [  # name, (H, W), quality, subsampling, r        (48 x 72 at 4:2:0: 15 MCUs; at 4:4:4: 54)
    ("r1_420_q90", (48, 72), 90, "4:2:0", 1),       # 15 intervals: RST0..RST7, RST0..RST5
    ("r3_444_q95", (48, 72), 95, "4:4:4", 3),       # 18 intervals
    ("r3_420_odd_q75", (41, 67), 75, "4:2:0", 3),   # partial MCUs, 15 MCUs -> 5 intervals
    ("r1_444_odd_q100", (33, 50), 100, "4:4:4", 1),  # 35 intervals
    ("r8_420_q90", (48, 64), 90, "4:2:0", 8),       # the round trip through the device decoder: 12 MCUs, 2 intervals
]


def main():
    out = os.path.join(HERE, "jpeg_encode")
    os.makedirs(out, exist_ok=True)
    for i, (name, (h, w), q, ss, r) in enumerate(CASES):
        rng = np.random.default_rng(7000 + i)
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(3 * xx + yy) % 256, (2 * yy + 40) % 256, (xx + 2 * yy + 90) % 256], -1)
        rgb = np.clip(smooth + rng.normal(0, 25, size=(h, w, 3)), 0, 255).astype(np.uint8)
        data = M.pil_encode(rgb, q, ss, r)
        np.savez_compressed(os.path.join(out, name + ".npz"), rgb=rgb, jpeg=np.frombuffer(data, np.uint8), quality=q, restart_mcus=r,
                            subsampling=ss)
        print(name, len(data))


if __name__ == "__main__":
    main()
