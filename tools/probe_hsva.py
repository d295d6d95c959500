"""Times spng_hsva_batch against the copy ceiling measured in the same process (profiles/r11_hsva.md):

    python tools/probe_hsva.py [--images 256] [--side 4096] [--repeats 5] [--out FILE]

`images` arrays of side^2 pixels, the three operations, on a raster of uniformly random bytes and on one whose pixels are all grey
(d = 0: no division; s = 0 on the way back: no sector arithmetic).  The HSVA inputs of the two TO operations are what FROM_RGBA8
made of the raster.  Kernel time comes from spng_profile (HIP events around the launch), the ceiling from spng_copy_ceiling pattern 0
over the same number of bytes (in + out).  Prints a markdown table."""
import argparse
import ctypes
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import swift_png_amd as spng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    s = spng.load(0)
    one = args.side * args.side                                 # pixels of an array
    total = one * args.images
    lines = [f"source digest {spng.source_digest()}, {args.images} arrays of {args.side}^2 pixels, {args.repeats} timed calls after one "
             f"warm-up", "", "| operation | raster | ms | GB/s (in + out) | copy ceiling GB/s | fraction | trapped |", "|---|---|---|---|---|---|---|"]
    # the ceilings first, on buffers of their own: (4 + 8) and (8 + 2) bytes per pixel, half of them read and half written
    ceiling = {}
    for per in (12, 10):
        half = total * per // 2
        a = torch.zeros(half, dtype=torch.uint8, device=s.tdev)
        b = torch.empty(half, dtype=torch.uint8, device=s.tdev)
        ms = ctypes.c_double(0)
        spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, b.data_ptr(), a.data_ptr(), half, 0, args.repeats, ctypes.byref(ms)))
        ceiling[per] = 2 * half / (ms.value * 1e-3) / 1e9
        del a, b
    torch.cuda.empty_cache()
    rgba = torch.randint(0, 256, (4 * total,), dtype=torch.uint8, device=s.tdev)
    hsva = torch.empty(8 * total, dtype=torch.uint8, device=s.tdev)
    back = torch.empty(4 * total, dtype=torch.uint8, device=s.tdev)
    cut = lambda t, per: [t[j * one * per:(j + 1) * one * per] for j in range(args.images)]
    runs = (("FROM_RGBA8", spng.HSVA_FROM_RGBA8, cut(rgba, 4), cut(hsva, 8), 12),
            ("TO_RGBA8", spng.HSVA_TO_RGBA8, cut(hsva, 8), cut(back, 4), 12),
            ("TO_VA8", spng.HSVA_TO_VA8, cut(hsva, 8), cut(back, 2), 10))
    for raster in ("random", "grey"):
        if raster == "grey":
            px = rgba.view(-1, 4)
            px[:, 1] = px[:, 0]
            px[:, 2] = px[:, 0]
        for name, op, ins, outs, per in runs:
            _, res = s.hsva_batch(ins, op, outs=outs)           # warm-up (and the HSVA input of the operations behind it)
            assert all(r.status == 0 for r in res)
            if name == "TO_RGBA8":
                assert torch.equal(back, rgba)                  # (the round trip, while it is there)
            s.profile(True)
            for _ in range(args.repeats):
                s.hsva_batch(ins, op, outs=outs)
            t, n = s.profile_get(spng.K_HSVA)
            s.profile(False)
            assert n == args.repeats
            t /= n
            rate = per * total / (t * 1e-3) / 1e9
            lines.append(f"| {name} | {raster} | {t:.3f} | {rate:.0f} | {ceiling[per]:.0f} | {rate / ceiling[per]:.2f} | "
                         f"{sum(r.aux[0] for r in res)} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
