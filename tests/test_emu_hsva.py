"""hsva_kernel of csrc/hsva.hip (the HSVA colour target of the reference's Snippets/PNG/CustomColor.swift:19-78, without an integer
division) run on the CPU by the wave emulator of tools/emu (host compiler: the ROCm clang++) against the tutorial's formulas restated
with plain `/` and `%` in tools/emu/emu_hsva.cpp: every colour forward, every colour there and back, and a grid of HSVA values."""
import subprocess

import pytest

import emu_build


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build_plain(tmp_path_factory, "hsva.hip", "emu_hsva.cpp", "EMU_HSVA_SRC", "-O2")


@pytest.mark.parametrize("mode", ["forward", "roundtrip", "grid"])
def test_emulated_hsva_kernel_matches_plain_division(emu, mode):
    """forward: SPNG_HSVA_FROM_RGBA8 over all 2^24 colours on the 16-byte path, a stride of them pixel by pixel.  roundtrip:
    SPNG_HSVA_TO_RGBA8 of it is the input and nothing traps.  grid: SPNG_HSVA_TO_RGBA8 / _TO_VA8 over the sector boundaries of h (k 65537 +
    {0, 1, 32768, 65535, 65536}, k = 0 ... 7, and 2^32 - 1), eight s and every v, aligned and not, and 2^20 random pixels; outputs, trap
    counts and the bytes around the output."""
    r = subprocess.run([str(emu), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (mode, r.stdout[-600:], r.stderr[-600:])
