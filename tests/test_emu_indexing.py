"""census_kernel, census_finish_kernel and pack_indexed_kernel of csrc/indexing.hip (the distinct UInt8 aggregates of a pixel array
and the pack through a key -> index map: the indexer closures of PNG.RGBA.swift:409-423, PNG.VA.swift:334-350 and
PNG.Image.swift:767-782 as tables) run on the CPU by the wave emulator of tools/emu (host compiler: the ROCm clang++) against
std::map in tools/emu/emu_indexing.cpp."""
import subprocess

import pytest

import emu_build


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build_plain(tmp_path_factory, "indexing.hip", "emu_indexing.cpp", "EMU_INDEXING_SRC", "-O2")


@pytest.mark.parametrize("mode", ["census", "pack"])
def test_emulated_indexing_kernels_match_a_map(emu, mode):
    """census: T = UInt8 / UInt16, three layouts; 0 ... 2051 pixels on one and three workgroups; a flat array; exactly cap and
    cap + 1 keys; the keys 0 and 0xFFFFFFFF; {k << s}; more distinct keys in one workgroup than its LDS table may hold, twice
    (the merge), on both sides of the sort's LDS limit; overflow seen early and late; both premultiplications; no counts; nothing
    written behind the result.  pack: the same sizes at storage offsets 0 ... 3, maps of 0 ... 65536 keys around the LDS
    threshold, misses counted, the keys 0 and 0xFFFFFFFF present and absent, the identity indexer, both premultiplications."""
    r = subprocess.run([str(emu), mode], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (mode, r.stdout[-600:], r.stderr[-600:])
