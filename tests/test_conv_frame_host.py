"""The frame of the persistent conv kernels, without a GPU: which workgroup computes which tile, the clamp of the device-side image
count and the border tap mask (csrc/conv_common.h: conv_tile_walk, conv_image_count, conv_tap_mask, conv_tap_mask_s1).

tests/native/conv_frame_harness.cpp prints what the functions return.  Every persistent kernel calls conv_tile_walk, every kernel that
takes n_dev calls conv_image_count; of the tap masks only conv_tap_mask_s1 has a kernel caller (the lab row-patch kernel): conv_mfma.hip
and conv3x3_lean.hip keep hand-written copies, which this test does NOT cover (the GPU parity tests do).  Everything is checked here,
against a restatement of the formulas in Python and against the properties the kernels rely on: every tile has exactly one owner,
a workgroup of a grid that is a multiple of 8 stays inside its XCD's eighth of the tile list, the tile counts of the workgroups of
an XCD differ by at most one.  Once plain, once with the address and undefined-behaviour sanitizers (host code, a stand-alone
program)."""
import os
import shutil
import subprocess
from collections import defaultdict

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "face-recognition-platform_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INT_MAX = 2**31 - 1

GRIDS_8 = [8, 64, 256, 512]
GRIDS_REST = [1, 5, 9, 36, 250, 255]
MAPS = [(1, 1), (1, 5), (2, 2), (3, 7), (8, 8)]
KINDS = [(3, 1), (3, 2), (1, 1), (1, 2)]                      # (KS, stride); pad = KS // 2


def tile_counts(G):
    return [0, 1, 7, 8, 9, G - 1, G, G + 1, 2 * G + 3, 8 * G, 100003]


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def printed(request, tmp_path_factory):
    """{kind: [rows of ints]} of the harness's output"""
    if hipcc() is None:
        pytest.skip("no hipcc here")
    sanitize = request.param
    tmp = tmp_path_factory.mktemp("conv_frame")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    obj, exe = str(tmp / "conv_frame_harness.o"), str(tmp / "conv_frame_harness")
    r = subprocess.run([hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-Wno-unused-function"] + san + ["-x", "hip", "-c", os.path.join(HERE, "native", "conv_frame_harness.cpp"), "-o", obj],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([hipcc()] + (["-Xarch_host", "-fsanitize=address,undefined"] if sanitize else []) + [obj, "-Wl,--unresolved-symbols=ignore-all", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rows = defaultdict(list)
    lines = r.stdout.split("\n")
    for line in lines[:-2]:
        kind, *vals = line.split()
        rows[kind].append([int(v) for v in vals])
    assert lines[-2] == f"lines {sum(len(v) for v in rows.values())}" and set(rows) == {"walk", "tap", "count"}
    return rows


# ---------------------------------------------------------------------------------------------------- tile walk
def walk_formula(n_tiles, G, b):
    """the kernels' formula as every family spelled it before it was shared (C integer division of non-negative values)"""
    if (G & 7) == 0:
        x, j, per = b & 7, b >> 3, G >> 3
        cs, ce = (x * n_tiles) // 8, ((x + 1) * n_tiles) // 8
        return cs + j, ce, per
    return (b * n_tiles) // G, ((b + 1) * n_tiles) // G, 1


def test_walk_gives_every_tile_exactly_one_owner(printed):
    walks = defaultdict(dict)
    for G, n, b, t0, t1, tstep in printed["walk"]:
        walks[(G, n)][b] = (t0, t1, tstep)
    assert set(walks) == {(G, n) for G in GRIDS_8 + GRIDS_REST for n in tile_counts(G)}
    for (G, n), per_b in walks.items():
        assert sorted(per_b) == list(range(G))
        owners = [0] * n
        counts = []
        for b, (t0, t1, tstep) in per_b.items():
            assert (t0, t1, tstep) == walk_formula(n, G, b), (G, n, b)
            assert tstep >= 1 and t0 >= 0 and t1 <= n, (G, n, b, t0, t1, tstep)
            tiles = range(t0, t1, tstep) if t0 < t1 else range(0)
            for tile in tiles:
                owners[tile] += 1
            counts.append(len(tiles))
            if G % 8 == 0:                                    # inside the XCD's eighth of the list
                x = b % 8
                assert all(x * n // 8 <= tile < (x + 1) * n // 8 for tile in tiles), (G, n, b)
        assert owners == [1] * n, (G, n, [i for i, c in enumerate(owners) if c != 1][:8])
        if G % 8 == 0:
            for x in range(8):
                of_xcd = counts[x::8]
                assert max(of_xcd) - min(of_xcd) <= 1, (G, n, x, of_xcd)
        else:                                                 # contiguous ranges: balanced over the whole grid
            assert max(counts) - min(counts) <= 1, (G, n, counts)


# ---------------------------------------------------------------------------------------------------- border taps
def tap_inside(oy, ox, H, W, stride, pad, KS, kh, kw):
    if kh >= KS or kw >= KS:
        return False
    y, x = oy * stride - pad + kh, ox * stride - pad + kw
    return 0 <= y < H and 0 <= x < W


def test_tap_mask_marks_exactly_the_taps_inside_the_image(printed):
    seen = set()
    for KS, stride, H, W, oy, ox, mask, *s1 in printed["tap"]:
        seen.add((KS, stride, H, W, oy, ox))
        want = sum(1 << (kh * 3 + kw) for kh in range(3) for kw in range(3) if tap_inside(oy, ox, H, W, stride, KS // 2, KS, kh, kw))
        assert mask == want, (KS, stride, H, W, oy, ox, bin(mask), bin(want))
        assert len(s1) == (1 if (KS, stride) == (3, 1) else 0)
        if s1:                                                # the stride-1 special case of the row-patch kernels
            assert s1[0] == mask, (H, W, oy, ox, bin(s1[0]), bin(mask))
    assert seen == {(KS, s, H, W, oy, ox) for KS, s in KINDS for H, W in MAPS for oy in range(H) for ox in range(W)}


# ---------------------------------------------------------------------------------------------------- image count
def test_image_count_stays_inside_the_capacity(printed):
    got = {(v, N): n for v, N, n in printed["count"]}
    for N in (1, 4, 32):
        for v, want in ((-3, 0), (0, 0), (1, 1), (N, N), (N + 1, N), (INT_MAX, N)):
            assert got[(v, N)] == want, (v, N, got[(v, N)])
