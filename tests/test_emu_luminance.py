"""luminance_kernel of csrc/luminance.hip (COMPUTE_LUMINANCE of the reference's Snippets/PNG/BasicEncoding.swift:63-71, binary64 up to the
sum and a float root settled against a table of doubles) run on the CPU by the wave emulator of tools/emu (host compiler: the ROCm
clang++) against the formula written plainly with sqrt and round in tools/emu/emu_luminance.cpp."""
import subprocess

import pytest

import emu_build


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build_plain(tmp_path_factory, "luminance.hip", "emu_luminance.cpp", "EMU_LUMINANCE_SRC", "-O2")


@pytest.mark.parametrize("mode", ["table", "v8", "va8"])
def test_emulated_luminance_kernel_matches_sqrt_and_round(emu, mode):
    """table: every entry of LUMINANCE_STEP is the smallest double whose rounded root reaches its index, and the function is right
    three doubles to either side of each.  v8 / va8: the operation over all 2^24 colours on the 16-byte path (alpha a byte of the
    index), and a stride of them on the 16-byte path with a tail, pixel by pixel and from an odd address; the bytes around the output
    and the job's result are untouched."""
    r = subprocess.run([str(emu), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (mode, r.stdout[-600:], r.stderr[-600:])
