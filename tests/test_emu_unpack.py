"""unpack_kernel and pack_kernel of csrc/unpack.hip, as written, run on the CPU by the wave emulator of tools/emu (host compiler: the
ROCm clang++) over the case table of tests/unpack_cases.py against the oracle's bytes (oracle/pixels.py), byte for byte, every output
between guard bytes: tools/emu/emu_unpack.cpp.  Twice: a plain build, and one with -fsanitize=address,undefined -- a CPU program of its
own, run as a subprocess, nothing preloaded --, which is what sees a tail that reads or writes one quad too far.

Left out here, and only here (tests/test_gpu_unpack_cases.py runs them on the device): the two cases of 4097 x 4096 pixels
(unpack_cases.HUGE): 16 Mi emulated threads' turns take minutes on a CPU, and what they add -- turns beyond the fourth under the capped
grid -- is the same loop the 1023 x 17 cases take four times.
The sanitizer build takes -fno-sanitize=alignment (why: tools/emu/emu_unpack.cpp); every other check is on for every case."""
import subprocess

import pytest

import emu_build
import unpack_cases as uc

LEFT_OUT = ["unpack/v8/u8/scalar/huge", "pack/v8/u8/scalar/huge"]
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")


def emulated():
    """the cases the emulator runs, those of one kernel and T behind one another (neighbours share a launch)"""
    assert sorted(LEFT_OUT) == sorted(c.name for c in uc.CASES if c.huge)
    return sorted((c for c in uc.CASES if c.name not in LEFT_OUT), key=lambda c: (c.kind, c.bits))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("unpack_cases")
    cases = emulated()
    uc.dump(d / "table.bin", d / "want.bin", cases)
    return d / "table.bin", d / "want.bin", cases


def test_emulated_kernels_match_the_oracle_on_every_case(tmp_path_factory, table):
    emu = emu_build.build_plain(tmp_path_factory, "unpack.hip", "emu_unpack.cpp", "EMU_UNPACK_SRC", "-O2")
    r = subprocess.run([str(emu), str(table[0]), str(table[1])], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("%d cases in " % len(table[2])) and ", 0 failed" in r.stdout


def test_emulated_kernels_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory, table):
    emu = emu_build.build_plain(tmp_path_factory, "unpack.hip", "emu_unpack.cpp", "EMU_UNPACK_SRC", "-O1", flags=SANITIZE + ("-DEMU_UCONTEXT",))
    r = subprocess.run([str(emu), str(table[0]), str(table[1])], capture_output=True, text=True, timeout=1800,
                       env={"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("%d cases in " % len(table[2])) and ", 0 failed" in r.stdout
