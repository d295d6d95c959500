"""Shared by tests/test_codegen*.py: a kernel source of swift_png_amd/csrc compiled to gfx950 assembly (no GPU needed: hipcc
cross-compiles) and the resources its metadata (amdhsa.kernels) states for every kernel.  A source is compiled once per session."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "max_flat_workgroup_size")


@functools.lru_cache(maxsize=None)
def kernel_table(name):
    """csrc/<name>.hip -> (the assembly text, {mangled kernel name: {key of KEYS: value}}).  Skips without hipcc."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(ROOT, "swift_png_amd", "csrc", name + ".hip")
        out = os.path.join(tmp, name + ".s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                       check=True, capture_output=True, timeout=900)
        asm = open(out).read()
    table = {}
    for blk in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels:"):])[1:]:
        def get(key, blk=blk):
            m = re.search(r"\." + key + r":\s+(\S+)", blk)
            return m.group(1) if m else "0"
        table[get("name")] = {k: int(get(k)) for k in KEYS}
    return asm, table
