"""Register budgets of the conv / stem kernels (no GPU needed: hipcc cross-compiles).  The kernels that share the conv epilogue
(conv_common.h) sit at their register limits - their header comments record what a handful of spilled registers cost - so a change to
the shared code is held to tests/golden/kernel_resources.json (tools/kernel_resources.py on the commit before the epilogue was shared):
per kernel no more scratch, no more spills and no lower occupancy.  The numbers belong to one compiler: another one skips."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def occupancy(vgpr_count):
    """Waves per SIMD the unified 512-register file admits (allocation granule 8)."""
    return 512 // ((vgpr_count + 7) // 8 * 8)


@pytest.fixture(scope="module")
def built():
    kr = _tool()
    assert os.path.exists(kr.HIPCC) or shutil.which(kr.HIPCC), "no hipcc here"
    version = kr.compiler_version()
    if version != GOLDEN["compiler"]:
        pytest.skip(f"the golden numbers are those of '{GOLDEN['compiler']}', this compiler is '{version}'")
    return kr.collect([(m, v["lab"]) for m, v in GOLDEN["modules"].items()])["modules"]


def test_golden_covers_the_guarded_set():
    assert {(m, v["lab"]) for m, v in GOLDEN["modules"].items()} == set(_tool().GUARDED)
    assert all(v["kernels"] for v in GOLDEN["modules"].values())


@pytest.mark.parametrize("module", sorted(GOLDEN["modules"]))
def test_kernel_resources_within_golden(built, module):
    gold, now = GOLDEN["modules"][module]["kernels"], built[module]["kernels"]
    assert set(now) == set(gold)
    for name, g in gold.items():
        n = now[name]
        print(name, "golden", g, "now", n)
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            assert n[field] <= g[field], (name, field, n[field], g[field])
        assert occupancy(n["vgpr_count"]) >= occupancy(g["vgpr_count"]), (name, n["vgpr_count"], g["vgpr_count"])
