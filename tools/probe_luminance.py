"""Times spng_luminance_batch against the copy ceiling measured in the same process (profiles/r12_luminance.md):

    python tools/probe_luminance.py [--images 64] [--side 4096] [--repeats 5] [--out FILE]

`images` arrays of side^2 RGBA8 pixels of uniformly random bytes, both operations.  Kernel time comes from spng_profile (HIP events
around the launch), the ceiling from spng_copy_ceiling pattern 0 over the same number of bytes (in + out).  SPNG_LIB names another
build of the library (tools/build_variant.sh WORK sqrt -DSPNG_LUMINANCE_SQRT: the compiler's binary64 root in place of the table);
the probe also compares every output byte of the first array with numpy's binary64 evaluation.  Prints a markdown table."""
import argparse
import ctypes
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import swift_png_amd as spng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    s = spng.load(0)
    one = args.side * args.side                                 # pixels of an array
    total = one * args.images
    lines = [f"library {spng.LIB_PATH.name}, source digest {spng.source_digest()}, {args.images} arrays of {args.side}^2 pixels, "
             f"{args.repeats} timed calls after one warm-up", "",
             "| operation | ms | GB/s (in + out) | Gpixel/s | copy ceiling GB/s | fraction | wrong bytes in the first array |", "|---|---|---|---|---|---|---|"]
    # the ceilings first, on buffers of their own: (4 + 1) and (4 + 2) bytes per pixel, half of them read and half written
    ceiling = {}
    for per in (5, 6):
        half = total * per // 2
        a = torch.zeros(half, dtype=torch.uint8, device=s.tdev)
        b = torch.empty(half, dtype=torch.uint8, device=s.tdev)
        ms = ctypes.c_double(0)
        spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, b.data_ptr(), a.data_ptr(), half, 0, args.repeats, ctypes.byref(ms)))
        ceiling[per] = 2 * half / (ms.value * 1e-3) / 1e9
        del a, b
    torch.cuda.empty_cache()
    rgba = torch.randint(0, 256, (4 * total,), dtype=torch.uint8, device=s.tdev)
    out = torch.empty(2 * total, dtype=torch.uint8, device=s.tdev)
    cut = lambda t, per: [t[j * one * per:(j + 1) * one * per] for j in range(args.images)]
    c = rgba[:4 * one].cpu().numpy().reshape(-1, 4).astype(np.float64)
    l = np.sqrt(((0.299 * c[:, 0]) * c[:, 0] + (0.587 * c[:, 1]) * c[:, 1]) + (0.114 * c[:, 2]) * c[:, 2])
    want = np.clip(np.floor(l) + (l - np.floor(l) >= 0.5), 0, 255).astype(np.uint8)
    for name, op in (("LUMINANCE_V8", spng.LUMINANCE_V8), ("LUMINANCE_VA8", spng.LUMINANCE_VA8)):
        ins, outs = cut(rgba, 4), cut(out, op)
        _, res = s.luminance_batch(ins, op, outs=outs)          # warm-up
        assert all(r.status == 0 for r in res)
        wrong = int((outs[0].cpu().numpy().reshape(-1, op)[:, 0] != want).sum())
        s.profile(True)
        for _ in range(args.repeats):
            s.luminance_batch(ins, op, outs=outs)
        t, n = s.profile_get(spng.K_LUMINANCE)
        s.profile(False)
        assert n == args.repeats
        t /= n
        rate = (4 + op) * total / (t * 1e-3) / 1e9
        lines.append(f"| {name} | {t:.3f} | {rate:.0f} | {total / (t * 1e-3) / 1e9:.0f} | {ceiling[4 + op]:.0f} | {rate / ceiling[4 + op]:.2f} | {wrong} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
