"""Shared by the tests/test_emu_*.py that emulate a kernel source as written: csrc/<source> prepared by prepare_plain of
tools/emu/prep_deflate.py (launches blanked, compiler-only barriers turned into meetings of the wave) and compiled for the CPU with its
driver of tools/emu."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU, CSRC = os.path.join(ROOT, "tools", "emu"), os.path.join(ROOT, "swift_png_amd", "csrc")
CLANG = os.environ.get("SPNG_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")


def build_plain(tmp_path_factory, source, driver, macro, opt, compiler=CLANG, flags=()):
    """the emulator of csrc/<source>: tools/emu/<driver> compiled at `opt` with -D<macro> naming the prepared source -> its path.
    Skips where the compiler is missing."""
    if not (os.path.exists(compiler) or shutil.which(compiler)):
        pytest.skip(os.path.basename(compiler) + " not available")
    sys.path.insert(0, EMU)
    import prep_deflate
    stem = os.path.splitext(driver)[0]
    d = tmp_path_factory.mktemp(stem)
    inc = d / (os.path.splitext(source)[0] + "_emu.inc")
    inc.write_text(prep_deflate.prepare_plain(open(os.path.join(CSRC, source)).read()))
    out = d / stem
    subprocess.run([compiler, opt, "-std=c++17", "-DSPNG_EMU", f'-D{macro}="{inc}"', "-I" + EMU, "-I" + CSRC, "-x", "c++", *flags, "-w",
                    "-o", str(out), os.path.join(EMU, driver)], check=True, capture_output=True, timeout=600)
    return out
