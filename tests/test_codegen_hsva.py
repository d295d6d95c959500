"""Code-generation guard for hsva_kernel (csrc/hsva.hip; no GPU needed: hipcc cross-compiles gfx950).  The kernel is meant to run at
the copy ceiling: 256 threads, no scratch, no spills, no LDS, and few enough registers for eight waves per SIMD."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "max_flat_workgroup_size")


def _kernels(name):
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
    return table


def test_hsva_kernel_resources():
    table = _kernels("hsva")
    ks = [v for k, v in table.items() if "hsva_kernel" in k]
    assert len(ks) == 1
    for v in ks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0
        assert v["group_segment_fixed_size"] == 0
        assert v["vgpr_count"] <= 64                            # eight waves per SIMD
        assert v["max_flat_workgroup_size"] == 256
