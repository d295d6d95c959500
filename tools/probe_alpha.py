"""Times spng_alpha_batch against the copy ceiling measured in the same process (profiles/r09_alpha.md):

    python tools/probe_alpha.py [--images 256] [--side 4096] [--repeats 5] [--out FILE]

`images` arrays of side^2 RGBA<UInt8> and RGBA<UInt16> pixels, out of place (the copy kernel reads one buffer and writes another
too), premultiply and straighten, on a raster of uniformly random bytes and on the same raster with every alpha set to T.max.
Kernel time comes from spng_profile (HIP events around the launch), the ceiling from spng_copy_ceiling pattern 0 over the same
number of bytes.  Prints a markdown table."""
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
    lines = [f"source digest {spng.source_digest()}, {args.images} arrays of {args.side}^2 pixels, out of place, "
             f"{args.repeats} timed calls after one warm-up", "",
             "| T | operation | alpha | ms | GB/s (in + out) | copy ceiling GB/s | fraction | trapped |", "|---|---|---|---|---|---|---|---|"]
    for bits in (8, 16):
        per = 4 * bits // 8
        one = args.side * args.side * per
        total = one * args.images
        src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=s.tdev)
        dst = torch.empty(total, dtype=torch.uint8, device=s.tdev)
        ms = ctypes.c_double(0)
        spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, dst.data_ptr(), src.data_ptr(), total, 0, args.repeats, ctypes.byref(ms)))
        ceiling = 2 * total / (ms.value * 1e-3) / 1e9
        for alpha in ("random", "T.max"):
            if alpha == "T.max":
                src.view(-1, per)[:, per - bits // 8:] = 255
            ins = [src[j * one:(j + 1) * one] for j in range(args.images)]
            outs = [dst[j * one:(j + 1) * one] for j in range(args.images)]
            for name, op in (("premultiply", spng.PREMULTIPLY), ("straighten", spng.STRAIGHTEN)):
                res = s.alpha_batch(ins, bits, spng.TARGET_RGBA, op, outs=outs)          # warm-up
                assert all(r.status == 0 for r in res)
                s.profile(True)
                for _ in range(args.repeats):
                    s.alpha_batch(ins, bits, spng.TARGET_RGBA, op, outs=outs)
                t, n = s.profile_get(spng.K_ALPHA)
                s.profile(False)
                assert n == args.repeats
                t /= n
                rate = 2 * total / (t * 1e-3) / 1e9
                lines.append(f"| UInt{bits} | {name} | {alpha} | {t:.3f} | {rate:.0f} | {ceiling:.0f} | {rate / ceiling:.2f} | "
                             f"{sum(r.aux[0] for r in res)} |")
        del src, dst
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
