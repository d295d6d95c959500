"""The kernels of csrc/colour_tables.hip (the wide census' gather, sort and write behind census_kernel of csrc/indexing.hip; the map's
build and lookup), as written, run on the CPU by the wave emulator of tools/emu (host compiler: the ROCm clang++) against std::map in
tools/emu/emu_colour_tables.cpp: the rules of tests/colour_table_cases.py up to 131 073 keys, every launch of a stage an emulated launch
of its own, every output between guard bytes.  Twice: a plain build, and one with -fsanitize=address,undefined -- a CPU program of its
own, run as a subprocess, nothing preloaded --, which is what sees a probe, a gather or a store one element too far.  The sanitizer
build runs every rule, and of the sizes above the old ceiling one each (65 537 keys; `brief`): it is some thirty times slower, and what
the larger sizes add is more turns of the same loops.
The sanitizer build takes -fno-sanitize=alignment, as tests/test_emu_unpack.py does: quad_keys reads unaligned quads through T."""
import os
import subprocess
import sys

import pytest

import emu_build

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")


def build(tmp_path_factory, opt, flags=()):
    """tools/emu/emu_colour_tables.cpp over prepared copies of both sources (emu_build prepares colour_tables.hip; indexing.hip, whose
    census_kernel is the counting stage, is prepared here the same way)"""
    sys.path.insert(0, emu_build.EMU)
    import prep_deflate
    inc = tmp_path_factory.mktemp("indexing_inc") / "indexing_emu.inc"
    inc.write_text(prep_deflate.prepare_plain(open(os.path.join(emu_build.CSRC, "indexing.hip")).read()))
    return emu_build.build_plain(tmp_path_factory, "colour_tables.hip", "emu_colour_tables.cpp", "EMU_COLOUR_TABLES_SRC", opt,
                                 flags=(f'-DEMU_INDEXING_SRC="{inc}"',) + tuple(flags))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build(tmp_path_factory, "-O2")


@pytest.fixture(scope="module")
def emu_sanitized(tmp_path_factory):
    return build(tmp_path_factory, "-O1", SANITIZE + ("-DEMU_UCONTEXT",))


@pytest.mark.parametrize("mode", ["census", "map"])
def test_emulated_colour_table_kernels_match_a_map(emu, mode):
    r = subprocess.run([str(emu), mode], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (mode, r.stdout[-600:], r.stderr[-600:])


@pytest.mark.parametrize("mode", ["census", "map"])
def test_emulated_colour_table_kernels_under_the_address_and_undefined_behaviour_sanitizers(emu_sanitized, mode):
    r = subprocess.run([str(emu_sanitized), mode, "brief"], capture_output=True, text=True, timeout=1800,
                       env={"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (mode, r.stdout[-2000:], r.stderr[-4000:])
