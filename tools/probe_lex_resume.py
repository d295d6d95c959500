"""Times the resumable chunk lexer beside the whole-file one (profiles/r14_lex_resume.md, profiles/r16_one_lexer.md):

    python tools/probe_lex_resume.py [--large 256] [--small 8192] [--huge 64] [--pieces 1,4,64] [--whole-only] [--package DIR] [--out FILE]

Three workloads: `large` copies of a file shaped like a 4K image's (30 MiB of IDAT in chunks of 64 KiB), `small` files of one 2 KiB
IDAT, and one file that is a single IDAT of `huge` MiB (0: left out), every file in device memory of its own.  Per workload: SPNG_K_LEX milliseconds (HIP events around the launches, spng_profile)
of spng_lex_batch once on the whole files; of spng_lex_resume_batch summed over the pushes when the files arrive in 1, 4 and 64 equal
pieces; and of spng_lex_batch on every growing prefix -- what a host had to do before, O(n k).  The counters of
spng_lex_resume_stats are printed beside the times: bytes summed and copied over all pushes do not depend on the pieces.
--whole-only: the first figure alone, with nothing the library did not have before (--package DIR: the package of another checkout,
to show that the whole-file entry did not move).  Prints a markdown table."""
import argparse
import ctypes
import struct
import sys
import zlib
from pathlib import Path


def chunk(name, data):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data))


def make_file(idat_bytes, chunk_bytes, seed):
    import numpy as np
    body = np.random.default_rng(seed).integers(0, 256, idat_bytes, dtype=np.uint8).tobytes()
    ihdr = chunk(b"IHDR", struct.pack(">IIBBBBB", 4096, 4096, 8, 6, 0, 0, 0))
    idats = b"".join(chunk(b"IDAT", body[i:i + chunk_bytes]) for i in range(0, idat_bytes, chunk_bytes))
    return b"\x89PNG\r\n\x1a\n" + ihdr + idats + chunk(b"IEND", b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", type=int, default=256)
    ap.add_argument("--small", type=int, default=8192)
    ap.add_argument("--huge", type=int, default=64)
    ap.add_argument("--pieces", default="1,4,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--package", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import swift_png_amd as spng
    import torch
    s = spng.load(0)
    lines = [f"library {spng.LIB_PATH}, source digest {spng.source_digest()}, best of {args.repeats} after one warm-up", ""]

    def timed(fn):
        """SPNG_K_LEX milliseconds of fn(), best of `repeats` after a warm-up"""
        fn()
        best = None
        for _ in range(args.repeats):
            s.profile(True)
            fn()
            ms, _ = s.profile_get(spng.K_LEX)
            s.profile(False)
            best = ms if best is None or ms < best else best
        return best

    for label, count, data in (("4K-image files", args.large, make_file(30 << 20, 1 << 16, 1)), ("small files", args.small, make_file(2048, 2048, 2)),
                               ("file of one IDAT", 1 if args.huge else 0, make_file(args.huge << 20, max(args.huge << 20, 1), 3))):
        if not count:
            continue
        n = len(data)
        png = s.to_device(data).repeat(count)                   # a copy per file
        idat = torch.empty(count * n, dtype=torch.uint8, device=s.tdev)
        descs = (spng.FileDesc * count)()
        infos = (spng.Lexed * count)()

        def whole(length):
            for i in range(count):
                descs[i] = spng.FileDesc(png.data_ptr() + i * n, length, idat.data_ptr() + i * n, n)
            spng._check(s.lib, s.lib.spng_lex_batch(s.ctx, descs, count, None, infos))
            return infos[0].status

        lines += [f"### {count} {label} of {n} bytes", "", "| how the files arrive | calls | SPNG_K_LEX ms | GB/s of file bytes | bytes summed | IDAT bytes copied | headers walked |",
                  "|---|---|---|---|---|---|---|"]
        ms = timed(lambda: whole(n))
        assert whole(n) == 0
        lines.append(f"| whole: spng_lex_batch | 1 | {ms:.3f} | {count * n / ms / 1e6:.0f} | | | |")
        if not args.whole_only:
            for k in [int(v) for v in args.pieces.split(",")]:
                cuts = [n * (j + 1) // k for j in range(k)]
                totals = [0, 0, 0]

                def pushed():
                    states = torch.zeros(count * int(s.lib.spng_lex_state_bytes()), dtype=torch.uint8, device=s.tdev)
                    sp = (ctypes.c_void_p * count)(*[states.data_ptr() + i * int(s.lib.spng_lex_state_bytes()) for i in range(count)])
                    totals[:] = [0, 0, 0]
                    for length in cuts:
                        for i in range(count):
                            descs[i] = spng.FileDesc(png.data_ptr() + i * n, length, idat.data_ptr() + i * n, n)
                        spng._check(s.lib, s.lib.spng_lex_resume_batch(s.ctx, descs, sp, count, None, infos))
                        for j, v in enumerate(s.lex_resume_stats()):
                            totals[j] += v
                    assert infos[0].status == 0 and infos[count - 1].status == 0

                ms = timed(pushed)
                lines.append(f"| {k} pieces: spng_lex_resume_batch | {k} | {ms:.3f} | {count * n / ms / 1e6:.0f} | {totals[0]} | {totals[1]} | {totals[2]} |")
                if k > 1:
                    ms = timed(lambda: [whole(length) for length in cuts])
                    lines.append(f"| {k} pieces: spng_lex_batch on every prefix | {k} | {ms:.3f} | {count * n / ms / 1e6:.0f} | | | |")
        lines.append("")
        del png, idat
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
