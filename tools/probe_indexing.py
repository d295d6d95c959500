"""Times spng_census_batch and spng_pack_indexed_batch against the copy ceiling measured in the same process
(profiles/r10_indexing.md):

    python tools/probe_indexing.py [--images 64] [--side 4096] [--repeats 5] [--bits 8,16] [--out FILE]

`images` arrays of side^2 RGBA<UInt8>, then RGBA<UInt16>, pixels in one call.  Census inputs: a flat colour, 256 colours with a
skewed histogram, 60 000 colours, uniformly random pixels (more than 65 536 colours: the early exit).  Mapped pack: maps of 256 and
60 000 keys, and next to them spng_pack_batch with the default indexer on the 256-colour image -- the existing kernel that does the
same memory work.  Kernel time comes from spng_profile (HIP events around the launches), the ceiling from spng_copy_ceiling
pattern 0 over the number of bytes the kernels read.  Prints a markdown table: bytes read per second as a fraction of the copy's
read + write rate."""
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
    ap.add_argument("--bits", default="8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    s = spng.load(0)
    n = args.side * args.side
    gen = torch.Generator(device=s.tdev)
    gen.manual_seed(10)

    def colours(k):                                             # k distinct keys as int32 bit patterns
        c = torch.unique(torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * k + 64,), dtype=torch.int64, device=s.tdev, generator=gen))
        return c[torch.randperm(len(c), device=s.tdev, generator=gen)[:k]].to(torch.int32)

    def image(kind):                                            # one image as n int32 keys
        if kind == "flat":
            return torch.full((n,), 0x40FF8040, dtype=torch.int32, device=s.tdev)
        if kind == "256 skewed":
            return colours(256)[(torch.rand(n, device=s.tdev, generator=gen) ** 3 * 256).long()]
        if kind == "60 000":
            return colours(60000)[torch.randint(0, 60000, (n,), device=s.tdev, generator=gen)]
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device=s.tdev, generator=gen).to(torch.int32)

    def pixels(keys, bits):                                     # `images` copies of the image, as T components
        if bits == 8:
            return keys.repeat(args.images)
        wide = (keys.view(torch.uint8).to(torch.int32) * 257).to(torch.int16)        # (component c -> c * 257: the key is c again)
        return wide.repeat(args.images)

    lines = [f"source digest {spng.source_digest()}, {args.images} arrays of {args.side}^2 pixels in one call, "
             f"{args.repeats} timed calls after one warm-up", "",
             "| T | kernel | input | ms | GB/s read | copy ceiling GB/s (read + write) | fraction | result |", "|---|---|---|---|---|---|---|---|"]

    def timed(kernel, call):
        call()
        s.profile(True)
        for _ in range(args.repeats):
            call()
        s.sync()
        t, k = s.profile_get(kernel)
        s.profile(False)
        assert k == args.repeats, k
        return t / k

    for bits in [int(b) for b in args.bits.split(",")]:
        per = 4 * bits // 8
        total = n * per * args.images
        a = torch.empty(total, dtype=torch.uint8, device=s.tdev)
        b = torch.empty(total, dtype=torch.uint8, device=s.tdev)
        ms = ctypes.c_double(0)
        spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, b.data_ptr(), a.data_ptr(), total, 0, args.repeats, ctypes.byref(ms)))
        ceiling = 2 * total / (ms.value * 1e-3) / 1e9
        del a, b

        def row(kernel, kind, t, result):
            rate = total / (t * 1e-3) / 1e9
            lines.append(f"| UInt{bits} | {kernel} | {kind} | {t:.3f} | {rate:.0f} | {ceiling:.0f} | {rate / ceiling:.2f} | {result} |")

        for kind in ("flat", "256 skewed", "60 000", "random"):
            px = pixels(image(kind), bits)
            one = px.numel() // args.images
            arrays = [px[j * one:(j + 1) * one] for j in range(args.images)]
            torch.cuda.synchronize()                            # (the context has a stream of its own: torch's kernels first)
            outs, res = s.census_batch(arrays, bits, spng.TARGET_RGBA, 65536)
            row("census", kind, timed(spng.K_CENSUS, lambda: s.census_batch(arrays, bits, spng.TARGET_RGBA, 65536)),
                f"status {res[0].status}, {res[0].written} keys")
            if kind in ("256 skewed", "60 000"):
                k = int(res[0].written)
                keys = [outs[0][0][:k]] * args.images
                idx = [(torch.arange(k, device=s.tdev) % 256).to(torch.uint8)] * args.images
                sto = [s.empty(n) for _ in range(args.images)]
                sizes = [(args.side, args.side)] * args.images
                torch.cuda.synchronize()
                _, pres = s.pack_indexed_batch(arrays, sizes, bits, spng.TARGET_RGBA, keys, idx, storages=sto)
                row("mapped pack", f"{kind}: map of {k} keys",
                    timed(spng.K_PACK_INDEXED, lambda: s.pack_indexed_batch(arrays, sizes, bits, spng.TARGET_RGBA, keys, idx, storages=sto)),
                    f"{sum(r.aux[0] for r in pres)} misses")
                if kind == "256 skewed":
                    pal = outs[0][0][:k].contiguous().view(torch.uint8)
                    torch.cuda.synchronize()
                    descs = (spng.PackDesc * args.images)()
                    for j in range(args.images):
                        descs[j] = spng.PackDesc(s._ptr(arrays[j]), s._ptr(sto[j]), s._ptr(pal), args.side, args.side, k, 8, 1, 1, 0, bits, 0, 0)
                    row("pack_kernel, default indexer", f"{kind}: palette of {k}",
                        timed(spng.K_PACK, lambda: spng._check(s.lib, s.lib.spng_pack_batch(s.ctx, descs, args.images))), "")
                del sto
            del px, arrays
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
