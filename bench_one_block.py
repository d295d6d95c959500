"""Inflate of streams that are ONE huge DEFLATE block (block cuts: swift_png_amd/csrc/pinflate2.hip), one JSON line.

Legs: 32 MiB of literals in one fixed block and ~64 MiB of output in one dynamic block, each as a single-stream spng_inflate_batch
call; a 4096 x 4096 RGBA8 image whose scanlines are one dynamic block (what an fpnge-style encoder writes) through spng_decode_batch,
alone and in a batch of 32.  Per leg, over the repeats (after warm-up calls): median and spread of the time of the parallel-inflate
pipeline between the HIP events the library records on its stream (spng_profile, SPNG_K_PINFLATE), MB/s of output by that median,
the medians of its decode and resolve stages and of the host's wall time, the nominal segment count and spng_cut_stats.  Where the library has block
cuts, the single-stream legs are measured once more under SPNG_BLOCK_CUT_NEVER as a cross-check; a library without them (an older
build: the baseline) runs the same legs through the exports it has.

Pushed legs (pushed_fixed, pushed_dynamic): the same two streams through spng_inflate_resume_batch, as 64 KiB and then 8 equal pieces,
the state handed from call to call.  Per leg: the sum over the pushes of the library's own HIP-event times (SPNG_K_PINFLATE +
SPNG_K_INFLATE: the pipeline and the serial kernel that takes what the pipeline leaves), median over the repeats, the same per
push, and spng_cut_stats per push.

    python bench_one_block.py [--repeats 7] [--warmup 2] [--legs fixed,dynamic,image1,image32,pushed_fixed,pushed_dynamic]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oneblock as ob           # noqa: E402  (the test-side one-block writers)
import swift_png_amd as spng    # noqa: E402


def timed(s, call, repeats, warmup):
    """-> per repeat: (pipeline ms, decode ms, resolve ms, wall ms).  The first three are HIP events the library records on its own
    stream around the parallel-inflate pipeline as a whole and around its decode and resolve stages (spng_profile); the wall time is
    the host's, call + synchronise, and for the image legs also holds the defilter."""
    import time
    for _ in range(warmup):
        call()
    s.sync()
    rows = []
    for _ in range(repeats):
        s.profile(True)
        t0 = time.perf_counter()
        call()
        s.sync()
        wall = (time.perf_counter() - t0) * 1e3
        rows.append((s.profile_get(spng.K_PINFLATE)[0], s.profile_get(spng.K_PINF_DECODE)[0], s.profile_get(spng.K_PINF_RESOLVE)[0], wall))
    s.profile(False)
    return rows


def summary(rows, out_bytes):
    pipe = [r[0] for r in rows]
    med = statistics.median(pipe)
    return {"ms": round(med, 3), "ms_min": round(min(pipe), 3), "ms_max": round(max(pipe), 3), "repeats": len(rows),
            "MB_per_s": round(out_bytes / 1e6 / (med * 1e-3), 1), "decode_ms": round(statistics.median(r[1] for r in rows), 3),
            "resolve_ms": round(statistics.median(r[2] for r in rows), 3), "wall_ms": round(statistics.median(r[3] for r in rows), 3)}


def segments(src_len):
    """NOMINAL segment count of a single-stream call: the automatic segment length of host_decode.hip's plan_inflate (geometry.hpp,
    `inflate_segment_bytes`), 64 .. 256 KiB, restated here without what the planner learns from the batch before (the library does
    not export the count)"""
    seg = max(src_len // 32768, min(max(src_len // 4096, 64 << 10), 256 << 10))
    seg = (seg + 255) & ~255
    return (src_len + seg - 1) // seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="fixed,dynamic,image1,image32")
    args = ap.parse_args()
    import torch
    s = spng.load(0)
    has_cuts = hasattr(s, "cut_stats") and hasattr(spng, "CFG_BLOCK_CUT_BYTES")
    out = {"bench": "one_block", "block_cuts": has_cuts, "device": torch.cuda.get_device_name(0)}
    legs = args.legs.split(",")

    def stream_leg(name, data, z):
        d_z = s.to_device(z)
        d_out = s.empty(len(data) + 64)
        desc = (spng.StreamDesc * 1)(spng.StreamDesc(d_z.data_ptr(), len(z), d_out.data_ptr(), len(data) + 64, spng.FORMAT_ZLIB, 0))
        dres = s.empty(64)
        torch.cuda.synchronize()

        def call():
            assert s.lib.spng_inflate_batch(s.ctx, desc, 1, ctypes.c_void_p(dres.data_ptr()), None) == 0

        def run(tag):
            rows = timed(s, call, args.repeats, args.warmup)
            r = spng.Result.from_buffer_copy(bytes(dres[:ctypes.sizeof(spng.Result)].cpu().numpy()))
            assert r.status == 0 and r.written == len(data), (name, r.status, r.written)
            assert bytes(d_out[:len(data)].cpu().numpy()) == data, name
            leg = summary(rows, len(data))
            leg.update({"in_bytes": len(z), "out_bytes": len(data), "segments_nominal": segments(len(z)), "pipeline": int(r.reserved)})
            if has_cuts:
                leg["cut_stats"] = list(s.cut_stats())
            out[tag] = leg

        run(name)
        if has_cuts:
            s.configure(spng.CFG_BLOCK_CUT_BYTES, spng.BLOCK_CUT_NEVER)
            try:
                run(name + "_never")
            finally:
                s.configure(spng.CFG_BLOCK_CUT_BYTES, 0)

    def pushed_leg(name, data, z):
        first, k = 65536, 8
        step = (len(z) - first + k - 1) // k
        ends = [first] + [min(len(z), first + (i + 1) * step) for i in range(k)]
        d_z = s.to_device(z)
        d_out = s.empty(len(data) + 64)
        torch.cuda.synchronize()

        def once():
            state, per, stats, res = (0, 0, 0, 0), [], [], None
            s.profile(True)
            before = 0.0
            for n in ends:
                res, state = s.inflate_resume(d_z, n, d_out, spng.FORMAT_ZLIB, state)
                assert res.status == (0 if n == len(z) else 1), (name, n, res.status)
                now = s.profile_get(spng.K_PINFLATE)[0] + s.profile_get(spng.K_INFLATE)[0]
                per.append(now - before)
                before = now
                if has_cuts:
                    stats.append(list(s.cut_stats()))
            s.profile(False)
            assert res.written == len(data) and res.consumed == len(z), name
            return per, stats

        for _ in range(args.warmup):
            once()
        runs = [once() for _ in range(args.repeats)]
        assert bytes(d_out[:len(data)].cpu().numpy()) == data, name
        totals = [sum(per) for per, _ in runs]
        med = statistics.median(totals)
        out[name] = {"ms": round(med, 3), "ms_min": round(min(totals), 3), "ms_max": round(max(totals), 3), "repeats": len(runs),
                     "MB_per_s": round(len(data) / 1e6 / (med * 1e-3), 1), "pushes": len(ends), "in_bytes": len(z), "out_bytes": len(data),
                     "ms_per_push": [round(statistics.median(per[i] for per, _ in runs), 3) for i in range(len(ends))],
                     "cut_stats_per_push": runs[-1][1]}

    if "pushed_fixed" in legs:
        pushed_leg("pushed_fixed_32MiB", *ob.one_fixed_block(11, 32 << 20))
    if "pushed_dynamic" in legs:
        pushed_leg("pushed_dynamic_64MiB", *ob.one_dynamic_block(7, 68 << 20))
    if "fixed" in legs:
        stream_leg("fixed_32MiB", *ob.one_fixed_block(11, 32 << 20))
    if "dynamic" in legs:
        stream_leg("dynamic_64MiB", *ob.one_dynamic_block(7, 68 << 20))
    if "image1" in legs or "image32" in legs:
        from swift_png_amd import synth
        W = H = 4096
        img = synth.image(3, W, H)
        S, U = spng.storage_size(W, H, 8, 4), spng.inflated_size(W, H, 8, 4, False)
        d_sto = s.to_device(img.tobytes())
        d_rows = s.empty(U)
        torch.cuda.synchronize()
        assert s.filter_batch([s.image_desc(None, d_rows, d_sto, W, H, 8, 4, False)])[0].status == 0
        rows = bytes(d_rows.cpu().numpy())
        z = ob.literal_block(rows)
        assert zlib.decompress(z) == rows
        d_z = s.to_device(z)
        for m in (1, 32):
            if f"image{m}" not in legs:
                continue
            d_back = s.empty(m * S)
            d_scan = s.empty(m * (U + 64))
            descs = (spng.ImageDesc * m)(*[spng.ImageDesc(d_z.data_ptr(), len(z), d_scan.data_ptr() + j * (U + 64), U + 64, d_back.data_ptr() + j * S,
                                                          W, H, 8, 4, 0, spng.FORMAT_ZLIB, 0) for j in range(m)])
            dres = s.empty(m * 64)
            torch.cuda.synchronize()

            def call():
                assert s.lib.spng_decode_batch(s.ctx, descs, m, ctypes.c_void_p(dres.data_ptr()), None) == 0

            rows = timed(s, call, args.repeats, args.warmup)
            for j in (0, m - 1):
                assert torch.equal(d_back[j * S:(j + 1) * S], d_sto), f"image {j} of {m}"
            leg = summary(rows, m * S)
            leg.update({"images": m, "in_bytes": len(z), "segments_nominal": segments(len(z)) if m == 1 else None})
            if has_cuts:
                leg["cut_stats"] = list(s.cut_stats())
            out[f"fpnge_4k_x{m}"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
