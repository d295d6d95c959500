"""Code-generation guard for alpha_kernel (csrc/alpha.hip; no GPU needed: hipcc cross-compiles gfx950).  The kernel is meant to run at
the copy ceiling: 256 threads, no scratch, no spills, no LDS, and few enough registers for eight waves per SIMD."""
from codegen_tools import kernel_table


def test_alpha_kernel_resources():
    _, table = kernel_table("alpha")
    ks = [v for k, v in table.items() if "alpha_kernel" in k]
    assert len(ks) == 2                                         # T = UInt8, UInt16
    for v in ks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0
        assert v["group_segment_fixed_size"] == 0
        assert v["vgpr_count"] <= 64                            # eight waves per SIMD
        assert v["max_flat_workgroup_size"] == 256


def test_fused_forms_keep_the_pack_and_unpack_kernels_free_of_scratch():
    _, table = kernel_table("unpack")
    ks = [v for k, v in table.items() if "pack_kernel" in k]    # pack_kernel and unpack_kernel, T = UInt8, UInt16
    assert len(ks) == 4
    for v in ks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0
        assert v["vgpr_count"] <= 128 and v["max_flat_workgroup_size"] == 256
