"""The detection tail's shared box arithmetic without a GPU (csrc/box_nms.h: box_area1, box_iou1 - what decode_nms_kernel,
pyramid_merge_kernel and the tracker's tk_key call).

tests/native/box_iou_harness.cpp runs the two functions on the host over seeded random box pairs and fixed edge pairs; every result must
equal tracks.iou, the host model the tracker is held to, as float32 values (a NaN equals a NaN), and the areas the model's own area
lines.  Once plain, once with the address and undefined-behaviour sanitizers (host code, a stand-alone program).

What this holds is the formula and the operand order against an independent restatement.  It does NOT hold the rule "one rounding per
operation": the host compiler fuses nothing in these two functions with or without the header's `#pragma clang fp contract(off)`, on a
CPU with FMA instructions too (the only product in front of a sum, inter = w * h, has a second use as the numerator), so the harness
prints the same bits either way.  On the device that rule is held by the array_equal tests of tests/test_gpu_kernels.py (decode),
tests/test_gpu_decode_exact.py (the planted cases of tests/decode_cases.py), tests/test_gpu_pyramid.py and tests/test_gpu_tracks.py, and for the callers' own box arithmetic by the Makefile's -ffp-contract=off
rule for the three files that include the header, which test_the_including_files_are_built_without_contraction holds in place.
test_kernel_budgets_of_the_detection_tail holds the kernels' LDS and scratch sizes (no GPU: the code objects' metadata)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from frp_amd import tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "face-recognition-platform_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
f32 = np.float32
N_RANDOM = 4000

NAN = float("nan")
EDGE_PAIRS = {
    "identical": ((10, 20, 50, 80), (10, 20, 50, 80)),
    "identical_fractional": ((10.25, 20.5, 50.125, 80.75), (10.25, 20.5, 50.125, 80.75)),
    "disjoint": ((0, 0, 10, 10), (100, 100, 120, 130)),
    "disjoint_in_x_only": ((0, 0, 10, 10), (40, 2, 60, 8)),
    "touching_by_one_pixel": ((0, 0, 10, 10), (10, 10, 20, 20)),           # the +1 convention: a 1 x 1 overlap
    "apart_by_one_pixel": ((0, 0, 10, 10), (11, 0, 20, 10)),               # xx2 - xx1 + 1 == 0
    "contained": ((0, 0, 100, 100), (25, 25, 50, 50)),
    "zero_size_both": ((5, 5, 5, 5), (5, 5, 5, 5)),
    "zero_size_inside": ((0, 0, 10, 10), (5, 5, 5, 5)),
    "zero_area": ((0, 0, -1, -1), (0, 0, -1, -1)),                          # (x2 - x1 + 1) == 0: 0 / 0
    "inverted_a": ((50, 20, 10, 80), (10, 20, 50, 80)),                     # x2 < x1
    "inverted_b": ((10, 20, 50, 80), (10, 80, 50, 20)),
    "inverted_both": ((50, 80, 10, 20), (50, 80, 10, 20)),
    "huge_a": ((-1e30, -1e30, 1e30, 1e30), (0, 0, 10, 10)),                 # infinite area
    "huge_both": ((-1e30, -1e30, 1e30, 1e30), (-1e30, -1e30, 1e30, 1e30)),  # inf / (inf - inf): NaN
    "huge_far": ((1e30, 1e30, 1e30, 1e30), (-1e30, -1e30, -1e30, -1e30)),
    "nan_a_x1": ((NAN, 0, 10, 10), (0, 0, 10, 10)),
    "nan_b_y2": ((0, 0, 10, 10), (0, 0, 10, NAN)),
    "nan_all": ((NAN, NAN, NAN, NAN), (NAN, NAN, NAN, NAN)),
    "inf_coordinate": ((0, 0, float("inf"), 10), (0, 0, 10, 10)),
}


def box_pairs():
    """[n, 8] float32: ax1 ay1 ax2 ay2 bx1 by1 bx2 by2 - the edge pairs, then detector-like random ones (half of them near copies
    of each other, so that the IoU covers its whole range, some with coordinates that do not round to pixels' fractions)"""
    rng = np.random.default_rng(20240607)
    xy = rng.uniform(-50, 1900, size=(N_RANDOM, 2, 2))
    wh = rng.uniform(-5, 400, size=(N_RANDOM, 2, 2))                         # a few inverted
    near = rng.random(N_RANDOM) < 0.5
    xy[near, 1] = xy[near, 0] + rng.normal(0, 12, size=(int(near.sum()), 2))
    wh[near, 1] = wh[near, 0] * rng.uniform(0.7, 1.4, size=(int(near.sum()), 2))
    rand = np.concatenate([xy, xy + wh], axis=2).reshape(N_RANDOM, 8)
    rand[::7] = np.round(rand[::7] * 4) / 4                                  # exact quarter pixels: exact ties are reachable
    edge = np.array([a + b for a, b in EDGE_PAIRS.values()], dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.concatenate([edge, rand]).astype(f32)


def model_area(x1, y1, x2, y2):
    """tracks.iou's area lines"""
    one = f32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(f32(x2 - x1) + one) * f32(f32(y2 - y1) + one))


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def pairs():
    return box_pairs()


@pytest.fixture(scope="module")
def model(pairs):
    """(area a, area b, iou) float32 arrays by the host model"""
    with np.errstate(over="ignore", invalid="ignore"):
        iou = np.array([tracks.iou(p[:4], p[4:]) for p in pairs], dtype=f32)
    aa = np.array([model_area(*p[:4]) for p in pairs], dtype=f32)
    ba = np.array([model_area(*p[4:]) for p in pairs], dtype=f32)
    return aa, ba, iou


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def printed(request, tmp_path_factory, pairs):
    """[n, 3] float32 of the harness's output: area a, area b, iou"""
    if hipcc() is None:
        pytest.skip("no hipcc here")
    sanitize = request.param
    tmp = tmp_path_factory.mktemp("box_iou")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    obj, exe = str(tmp / "box_iou_harness.o"), str(tmp / "box_iou_harness")
    r = subprocess.run([hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-Wno-unused-function"] + san + ["-x", "hip", "-c", os.path.join(HERE, "native", "box_iou_harness.cpp"), "-o", obj],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([hipcc()] + (["-Xarch_host", "-fsanitize=address,undefined"] if sanitize else []) + [obj, "-Wl,--unresolved-symbols=ignore-all", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    text = "".join(" ".join(f"{w:08x}" for w in row) + "\n" for row in pairs.view(np.uint32).tolist())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]                                  # a sanitizer's report
    lines = r.stdout.split("\n")
    assert lines[-2] == f"lines {len(pairs)}" and lines[-1] == "" and len(lines) == len(pairs) + 2
    return np.array([[int(w, 16) for w in line.split()] for line in lines[:-2]], dtype=np.uint32).view(f32)


def test_the_pairs_are_the_ones_named(pairs, model):
    """the inputs reach what they are meant to reach, by the model"""
    assert len(pairs) == len(EDGE_PAIRS) + N_RANDOM and N_RANDOM >= 2000
    iou = dict(zip(EDGE_PAIRS, model[2][:len(EDGE_PAIRS)]))
    area = dict(zip(EDGE_PAIRS, model[0][:len(EDGE_PAIRS)]))
    assert iou["identical"] == 1 and iou["identical_fractional"] == 1 and iou["zero_size_both"] == 1
    assert iou["disjoint"] == 0 and iou["disjoint_in_x_only"] == 0 and iou["apart_by_one_pixel"] == 0
    assert iou["touching_by_one_pixel"] == f32(1) / f32(241) and area["zero_size_both"] == 1
    assert np.isnan(iou["zero_area"]) and area["zero_area"] == 0
    assert area["inverted_a"] < 0 and area["inverted_both"] > 0
    assert np.isinf(area["huge_a"]) and iou["huge_a"] == 0 and np.isnan(iou["huge_both"])
    assert np.isnan(area["nan_a_x1"]) and np.isnan(iou["nan_a_x1"]) and np.isnan(iou["nan_b_y2"]) and np.isnan(iou["nan_all"])
    rand = model[2][len(EDGE_PAIRS):]
    assert (rand == 0).sum() > 100 and ((rand > 0) & (rand < 0.3)).sum() > 100 and (rand > 0.6).sum() > 100        # the whole range
    assert (pairs[len(EDGE_PAIRS):, 2] < pairs[len(EDGE_PAIRS):, 0]).any()                  # inverted boxes among the random ones


def _differing(got, want):
    """the first few (pair, harness, model) that differ, for the assertion's message"""
    return [(int(i), got[i], want[i]) for i in np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]]


def test_area_equals_the_host_model(printed, model):
    for col in (0, 1):
        assert np.array_equal(printed[:, col], model[col], equal_nan=True), _differing(printed[:, col], model[col])


def test_iou_equals_the_host_model(printed, model):
    got, want = printed[:, 2], model[2]
    assert got.dtype == want.dtype == f32
    assert np.array_equal(got, want, equal_nan=True), _differing(got, want)


def test_the_including_files_are_built_without_contraction():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    includers = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")) and '#include "box_nms.h"' in open(os.path.join(CSRC, f)).read())
    assert includers == ["decode_nms", "pyramid_kernels", "track_kernels"]
    for m in includers:
        assert "-ffp-contract=off" in kernel_resources.makefile_flags(m), m


# the issue's budgets: LDS equal to, scratch no more than, the figures of the commit before the tail was shared (this compiler)
BUDGETS = {"decode_nms": ("decode_nms_kernel", 46672, 56), "pyramid_kernels": ("pyramid_merge_kernel", 15368, 0),
           "track_kernels": ("track_associate_kernel", 8192, 0)}


def test_kernel_budgets_of_the_detection_tail():
    """pyramid_merge_kernel's figure depends on the order the compiler gives its two LDS variables (the alignas on `keys` in
    pyramid_kernels.hip steers it): another toolchain may lay them out differently, and this is where that shows"""
    if hipcc() is None:
        pytest.skip("no hipcc here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources.collect([(m, False) for m in BUDGETS], fields=kernel_resources.LDS_FIELDS)["modules"]
    for m, (kernel, lds, scratch) in BUDGETS.items():
        (name, r), = [(n, r) for n, r in res[m]["kernels"].items() if kernel in n]
        assert r["group_segment_fixed_size"] == lds and r["private_segment_fixed_size"] <= scratch, (name, r)
        assert r["vgpr_spill_count"] == 0, (name, r)
    for m in res:                                             # no kernel of the three files spills a vector register
        for name, r in res[m]["kernels"].items():
            assert r["vgpr_spill_count"] == 0, (name, r)
