"""Code-generation guard for luminance_kernel (csrc/luminance.hip; no GPU needed: hipcc cross-compiles gfx950).  256 threads, no
scratch, no spills, the table of steps as its only LDS.  The register bound is the built kernel's: 46 VGPRs -- the binary64 values
take register pairs --, which the allocation granule of 8 makes 48 (profiles/r12_luminance.md); eight waves per SIMD fit up to 64."""
from codegen_tools import kernel_table


def test_luminance_kernel_resources():
    asm, table = kernel_table("luminance")
    ks = [v for k, v in table.items() if "luminance_kernel" in k]
    assert len(ks) == 1
    for v in ks:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0
        assert v["group_segment_fixed_size"] == 257 * 8         # LUMINANCE_STEP
        assert v["vgpr_count"] <= 48
        assert v["max_flat_workgroup_size"] == 256
