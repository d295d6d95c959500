"""Host cost of a colour-target call (profiles/r12_colour_host.md): the mean wall time of consecutive spng_alpha_batch calls, and of as many
spng_hsva_batch calls, on one array of 16 RGBA<UInt8> pixels -- a size at which the kernel is nothing and the host layer everything.
The calls are asynchronous (results to the device); the clock runs around the loop and stops after sync().

    SPNG_LIB=variants/libspng_<name>.so python tools/probe_colour_host.py [--calls 2000] [--warmup 200]"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import swift_png_amd as spng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    s = spng.load(0)
    src, dst, d_res = s.to_device(bytes(range(64))), s.empty(128), s.empty(64)
    alpha = (spng.AlphaDesc * 1)(spng.AlphaDesc(src.data_ptr(), src.data_ptr(), 16, 8, spng.TARGET_RGBA, spng.PREMULTIPLY))
    hsva = (spng.HsvaDesc * 1)(spng.HsvaDesc(src.data_ptr(), dst.data_ptr(), 16, spng.HSVA_FROM_RGBA8))
    out = [spng.LIB_PATH.name]
    for name, entry, descs in (("alpha_batch", s.lib.spng_alpha_batch, alpha), ("hsva_batch", s.lib.spng_hsva_batch, hsva)):
        for n in (args.warmup, args.calls):
            s.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                spng._check(s.lib, entry(s.ctx, descs, 1, d_res.data_ptr(), None))
            s.sync()
            us = (time.perf_counter() - t0) / max(n, 1) * 1e6
        out.append(f"{name} {us:.2f} us per call")
    print(", ".join(out))


if __name__ == "__main__":
    main()
