"""The fused residual-block kernel's work decomposition and code object, without a GPU.

tests/native/block64_plan_harness.cpp links csrc/conv3x3_block64.hip compiled host-only and walks the plan function and the item
function - the ones the launcher and the kernel evaluate - over the maps of tests/test_gpu_block64.py and the headline shapes: every
output pixel has exactly one owner, every item stays within the declared halo, LDS <= 160 KiB, shapes beyond signed 32-bit byte offsets
are refused.  Once plain, once built with the address and undefined-behaviour sanitizers (host code only, a stand-alone program).  The cross-compiled code object must use no
scratch, spill no register and stay within 256 vector registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "face-recognition-platform_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def build(out_dir, sanitize):
    os.makedirs(out_dir, exist_ok=True)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    flags = ["-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
             "-Wno-unused-function"] + san
    objs = []
    for src in (os.path.join(CSRC, "conv3x3_block64.hip"), os.path.join(HERE, "native", "block64_plan_harness.cpp")):
        objs.append(os.path.join(out_dir, os.path.basename(src) + ".o"))
        r = subprocess.run([hipcc()] + flags + ["-x", "hip", "-c", src, "-o", objs[-1]], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
    exe = os.path.join(out_dir, "block64_plan_harness")
    r = subprocess.run([hipcc()] + (["-Xarch_host", "-fsanitize=address,undefined"] if sanitize else []) + objs + ["-rdynamic", "-ldl", "-Wl,--unresolved-symbols=ignore-all", "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_covers_every_pixel_once_and_stays_in_reach(tmp_path, sanitize):
    if hipcc() is None:
        pytest.skip("no hipcc here")
    exe = build(str(tmp_path), sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for ncu in (256, 64, 0):
        r = subprocess.run([exe, str(ncu)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("all ok"), (ncu, r.stdout[-2000:], r.stderr[-4000:])
    lines = {tuple(int(v) for v in re.findall(r"[NHW]=(\d+)", l)): l for l in r.stdout.splitlines() if l.startswith("ok ")}
    assert "segs=1 " in lines[(32, 272, 480)] and "items=512" in lines[(32, 272, 480)]          # two whole rounds of whole strips


def test_code_object_uses_no_scratch_and_at_most_256_registers(tmp_path):
    readelf = shutil.which("llvm-readelf") or (os.path.exists("/opt/rocm/llvm/bin/llvm-readelf") and "/opt/rocm/llvm/bin/llvm-readelf")
    if hipcc() is None or not readelf:
        pytest.skip("no hipcc / llvm-readelf here")
    co = str(tmp_path / "block64.co")
    r = subprocess.run([hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-Wno-unused-function", "-c", os.path.join(CSRC, "conv3x3_block64.hip"), "-o", co], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"\.name:\s+(\S*conv3x3_block64_kernel\S*)", notes)
    assert len(set(kernels)) == 2, kernels
    for field, limit in ((".private_segment_fixed_size", 0), (".vgpr_spill_count", 0), (".sgpr_spill_count", 0), (".vgpr_count", 256)):
        vals = [int(v) for v in re.findall(re.escape(field) + r":\s+(\d+)", notes)]
        assert len(vals) == 2 and max(vals) <= limit, (field, vals)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert max(lds) == 0                                                                        # (all of it dynamic: BLOCK64_LDS_BYTES)
