"""Code-generation guard for hsva_kernel (csrc/hsva.hip; no GPU needed: hipcc cross-compiles gfx950).  The kernel is meant to run at
the copy ceiling: 256 threads, no scratch, no spills, no LDS, and few enough registers for eight waves per SIMD."""
from codegen_tools import kernel_table


def test_hsva_kernel_resources():
    _, table = kernel_table("hsva")
    ks = [v for k, v in table.items() if "hsva_kernel" in k]
    assert len(ks) == 1
    for v in ks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0
        assert v["group_segment_fixed_size"] == 0
        assert v["vgpr_count"] <= 64                            # eight waves per SIMD
        assert v["max_flat_workgroup_size"] == 256
