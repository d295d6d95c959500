"""alpha_kernel of csrc/alpha.hip (premultiplied <-> straight alpha: PNG.premultiply / PNG.straighten, Sources/PNG/PNG.swift:55-117,
without an integer division) run on the CPU by the wave emulator of tools/emu (host compiler: the ROCm clang++) against the
formulas restated with plain `/` in tools/emu/emu_alpha.cpp: exhaustively at 8 bits, every alpha at 16 bits, and the whole
numerator range of the divide-by-T.max identity."""
import subprocess

import pytest

import emu_build


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build_plain(tmp_path_factory, "alpha.hip", "emu_alpha.cpp", "EMU_ALPHA_SRC", "-O2")


@pytest.mark.parametrize("mode", ["grid8", "sweep16", "divmax"])
def test_emulated_alpha_kernel_matches_plain_division(emu, mode):
    """grid8: all 65536 (c, a) pairs, four operations (the (as: UInt8.self) forms on 16-bit input), both layouts, aligned and not,
    in and out of place, with the trap count.  sweep16: every 16-bit alpha with the components around it and random ones.
    divmax: x / (2^k - 1) == (x + 1 + (x >> k)) >> k for every numerator c * a + (M >> 1) can be, k = 8 and 16."""
    r = subprocess.run([str(emu), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (mode, r.stdout[-600:], r.stderr[-600:])
