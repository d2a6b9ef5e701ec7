#!/usr/bin/env python3
"""Register budgets of the conv / stem kernels, without a GPU: compiles .hip files for gfx950 (device pass only, to assembly, with the
Makefile's flags) and reads each kernel's resource record from the code object metadata - nothing else of the assembly is looked at.

  tools/kernel_resources.py                          the guarded set (GUARDED below) -> JSON on stdout
  tools/kernel_resources.py -o FILE                  ... into FILE (tests/golden/kernel_resources.json was written this way)
  tools/kernel_resources.py [--lab] a.hip b.hip      these files (--lab: with -DFRP_LAB)
  tools/kernel_resources.py --lds a.hip              ... with each kernel's static LDS size (group_segment_fixed_size) as well

The numbers are properties of one compiler: its version line is part of the output.  tests/test_kernel_resources_host.py compares the
working tree with the golden file.
"""
import argparse
import concurrent.futures
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-recognition-platform_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (module, lab build): every kernel family that shares the conv epilogue (conv_common.h)
GUARDED = [("conv_mfma", False), ("conv3x3_lean", False), ("conv3x3_wino", False), ("conv3x3_c64", False), ("conv3x3_block64", False),
           ("conv3x3_s2", False), ("stem_kernel", False), ("conv3x3_rows", True)]
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")
LDS_FIELDS = FIELDS + (".group_segment_fixed_size",)     # (not in the golden file of the guarded set, which was written without it)


def makefile_flags(module, lab=False, csrc=CSRC):
    """The compile flags csrc/Makefile gives <module>.hip (CXXFLAGS, -ffp-contract=off for the objects it names, -DFRP_LAB for `make lab`)."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    root = os.path.abspath(os.path.join(csrc, "..", ".."))
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).replace("$(ROOT)", root).split()
    for rule in re.finditer(r"^(\$\(OBJ\)/\S+\.o(?:[ \t]+\$\(OBJ\)/\S+\.o)*):.*\n\t(.*)$", text, re.M):
        if f"$(OBJ)/{module}.o" in rule.group(1).split():
            flags += [f for f in rule.group(2).split() if f.startswith("-f")]
    return flags + (["-DFRP_LAB"] if lab else [])


def compiler_version():
    out = subprocess.run([HIPCC, "--version"], check=True, capture_output=True, text=True).stdout
    return next(line.strip() for line in out.splitlines() if "clang version" in line)


def parse_metadata(asm, fields=FIELDS):
    """{kernel name: {field: int}} from the .amdgpu_metadata block (amdhsa.kernels: one list item per kernel, keys at one indent)."""
    block = re.search(r"^\s*\.amdgpu_metadata\n(.*?)^\s*\.end_amdgpu_metadata", asm, re.M | re.S).group(1)
    kernels, cur = {}, None
    for line in block.splitlines():
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip()
        if key == ".name":
            kernels[val.strip("'\"")] = cur
        elif key in fields:
            cur[key[1:]] = int(val)
    return {k: v for k, v in kernels.items() if len(v) == len(fields)}


def module_resources(module, lab=False, csrc=CSRC, fields=FIELDS):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, module + ".s")
        cmd = [HIPCC] + makefile_flags(module, lab, csrc) + ["-S", "--cuda-device-only", "-o", out, os.path.join(csrc, module + ".hip")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        if r.returncode:
            raise RuntimeError(f"{module}.hip does not compile:\n{r.stderr[-4000:]}")
        return parse_metadata(open(out).read(), fields)


def collect(modules=GUARDED, csrc=CSRC, jobs=None, fields=FIELDS):
    jobs = jobs or min(len(modules), 8, os.cpu_count() or 1)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        res = list(pool.map(lambda ml: module_resources(ml[0], ml[1], csrc, fields), modules))
    return {"compiler": compiler_version(),
            "modules": {m: {"lab": lab, "kernels": dict(sorted(k.items()))} for (m, lab), k in zip(modules, res)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help=".hip files of csrc/ (default: the guarded set)")
    ap.add_argument("--lab", action="store_true", help="compile the named files with -DFRP_LAB")
    ap.add_argument("--lds", action="store_true", help="add group_segment_fixed_size to every kernel's record")
    ap.add_argument("--csrc", default=CSRC, help="source directory (with its Makefile)")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    modules = [(os.path.splitext(os.path.basename(f))[0], a.lab) for f in a.files] or GUARDED
    text = json.dumps(collect(modules, a.csrc, fields=LDS_FIELDS if a.lds else FIELDS), indent=1) + "\n"
    if a.output:
        open(a.output, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
