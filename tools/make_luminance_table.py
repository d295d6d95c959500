"""Prints LUMINANCE_STEP of swift_png_amd/csrc/luminance.hpp: for k = 0 ... 255 the smallest binary64 x >= 0 whose correctly rounded
square root, rounded to the nearest integer with halves away from zero, is at least k (Snippets/PNG/BasicEncoding.swift:63-71 of the
reference rounds so), found by bisection over the bit patterns; entry 256 is +infinity.  An entry is (k - 0.5)^2 or the double in
front of it: the root of the latter rounds up to k - 0.5 where (k - 0.5)^2 lies in the lower half of its power of four.

    python tools/make_luminance_table.py > table.inc        (tools/emu/emu_luminance.cpp checks the table in the header again)"""
import struct

import numpy as np


def rounded_root(x: float) -> int:
    l = np.sqrt(np.float64(x))
    whole = np.floor(l)
    return int(whole) + (1 if l - whole >= 0.5 else 0)


def bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<q", b))[0]


def step(k: int) -> float:
    if k == 0:
        return 0.0
    lo, hi = bits(0.0), bits(float(k * k))                      # rounded_root(lo) < k <= rounded_root(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rounded_root(from_bits(mid)) >= k:
            hi = mid
        else:
            lo = mid
    return from_bits(hi)


def main():
    cells = [step(k).hex() for k in range(256)]
    for at in range(0, 256, 4):
        print("    " + ", ".join(cells[at:at + 4]) + ",")
    print("    __builtin_inf()")


if __name__ == "__main__":
    main()
