"""Code-generation guard for the kernels of csrc/colour_tables.hip (no GPU needed: hipcc cross-compiles gfx950): no scratch, no
spills, and the workgroup size each is launched with.  Registers and LDS bytes are printed (pytest -s) for
profiles/r13_colour_tables.md; no figure that nobody has measured on the device is asserted."""
import os
import re

import pytest

from codegen_tools import ROOT, kernel_table

# kernel -> (instantiations, threads per workgroup at its launches in launch_census_wide_finish / launch_map)
LAUNCHED = {"census_gather_kernel": (1, 256), "census_sort_tile_kernel": (1, 1024), "census_sort_step_kernel": (1, 256),
            "census_write_kernel": (1, 256), "map_build_kernel": (1, 256), "map_kernel": (2, 256)}


@pytest.fixture(scope="module")
def kernels():
    return {name: v for name, v in kernel_table("colour_tables")[1].items() if "_kernel" in name}


def test_every_kernel_is_known_and_free_of_scratch(kernels):
    seen = {name: 0 for name in LAUNCHED}
    for mangled, v in kernels.items():
        name = next((n for n in sorted(LAUNCHED, key=len, reverse=True) if n in mangled), None)
        assert name is not None, f"{mangled}: a kernel this test does not know"
        seen[name] += 1
        print(f"{mangled}: {v['vgpr_count']} VGPRs, {v['sgpr_count']} SGPRs, {v['group_segment_fixed_size']} bytes of LDS")
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, mangled
        assert v["max_flat_workgroup_size"] == LAUNCHED[name][1], mangled
    assert seen == {name: n for name, (n, _) in LAUNCHED.items()}


def test_launches_use_the_declared_workgroup_sizes():
    src = open(os.path.join(ROOT, "swift_png_amd", "csrc", "colour_tables.hip")).read()
    launches = re.findall(r"\b(\w+_kernel)(?:<\w+>)?<<<[^;]*?\),\s*(\d+),|\b(\w+_kernel)(?:<\w+>)?<<<\s*\w+,\s*(\d+),", src)
    launches = [(a or c, b or d) for a, b, c, d in launches]
    assert len(launches) == 8
    for name, threads in launches:
        assert int(threads) == LAUNCHED[name][1], name
        assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (LAUNCHED[name][1], name), src), name
