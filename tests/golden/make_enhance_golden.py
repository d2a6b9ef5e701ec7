#!/usr/bin/env python3
"""Golden values for enhanced_size (face_service.py, tests/enhance_model.py) from the reference's own
backend/app/services/enhancer.py::_safe_resize_params (:49-62).

Runs only in the build container: `make_enhance_golden.py <reference>/backend`.  The module's logger import is the only thing
it needs from the application; MAX_PIXELS is the module constant the cases set.
Output: tests/golden/enhance_sizes.json (inputs + the reference's outputs, data only)."""
import json
import os
import sys
import tempfile

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "enhance_sizes.json")
# w, h, upscale factor, pixel cap
CASES = [
    (1920, 1080, 2.0, 4_000_000),        # the reference's defaults on the workload's frame: capped
    (3840, 2160, 2.0, 4_000_000),        # already above the cap: scaled down, so nothing is resampled
    (97561, 41, 2.0, 4_000_000),         # 4,000,001 pixels: one above the cap
    (97561, 41, 1.0, 4_000_000),
    (5, 3, 1.5, 4_000_000),              # 7.5 and 4.5: round() goes to the even neighbour
    (160, 160, 2.0, 4_000_000),          # a face crop: plain x2
    (160, 90, 2.0, 27_750),              # the non-integer ratio of a cap: 222 x 125
    (1, 1, 2.0, 4_000_000),
    (640, 480, 2.0, 1_228_800),          # exactly at the cap: not above it
    (640, 480, 2.0, 1_228_799),
]


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    os.chdir(tempfile.mkdtemp())                      # (the application's logger opens logs/ under the working directory)
    from app.services import enhancer
    rows = []
    for w, h, f, cap in CASES:
        enhancer.MAX_PIXELS = cap
        nw, nh = enhancer._safe_resize_params(w, h, f)
        rows.append({"w": w, "h": h, "upscale": f, "max_pixels": cap, "new_w": int(nw), "new_h": int(nh)})
    with open(OUT, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
    print(f"wrote {OUT}: {len(rows)} cases")


if __name__ == "__main__":
    main()
