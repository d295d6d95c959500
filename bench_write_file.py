"""bench_write_file.py -- the file writer (spng_write_file_batch) beside the IDAT writer it grew out of (spng_write_idat_batch) and
the library's copy ceiling, on the same bytes resident in HBM:

    many    256 streams of 1 MiB of random bytes, IDAT chunks of 65544 bytes (where the reference cuts at its default hint)
    one     the same 256 MiB as ONE stream written as ONE IDAT (chunk_bytes = 0x7fffffff): 1 MiB pieces, a wave each, folded

Timing by the context's profile timer (HIP events around the launches, SPNG_K_LEX), one step at a time: median of `--steps` steps (at
least 9) after `--warmup`, with the spread (min, max) the steps showed.  The new writer is also run with the lengths read from
spng_result records on the device, the form spng_compress_batch uses.  After the clock the IDAT chunks of both writers are compared
byte for byte.  Prints one JSON line.

    python bench_write_file.py [--steps 11] [--warmup 2] [--streams 256] [--mib 1]"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics

CHUNK = 65544


def timed(s, spng, call, steps, warmup):
    """-> (median ms, min ms, max ms) of `call` by the profile timer, a step at a time"""
    for _ in range(warmup):
        call()
    s.sync()
    ms = []
    for _ in range(steps):
        s.profile(True)
        call()
        s.sync()
        ms.append(s.profile_get(spng.K_LEX)[0])
    s.profile(False)
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--mib", type=int, default=1)
    ap.add_argument("--old-one-steps", type=int, default=3, help="steps of the old kernel on the one-chunk case (one wave: seconds per step)")
    a = ap.parse_args()
    steps = max(a.steps, 9)
    import torch
    import swift_png_amd as spng
    s = spng.load(0)
    n, each = a.streams, a.mib << 20
    total = n * each
    g = torch.Generator(device=s.tdev).manual_seed(15)
    data = torch.randint(0, 256, (total,), dtype=torch.uint8, device=s.tdev, generator=g)
    desc, keep = spng.png_desc((4096, 4096), 8, 4, chunk_bytes=CHUNK)
    head = int(s.lib.spng_file_bound(ctypes.byref(desc), each)) - each - 12 * -(-each // CHUNK) - 20
    out = {"bytes": total, "streams": n, "stream_bytes": each, "steps": steps, "warmup": a.warmup, "head_bytes": head}

    def chunking(count, length, chunk_bytes):
        cap = length + 12 * -(-length // chunk_bytes)
        dst = s.empty(count * cap)
        arr = (spng.ChunkingDesc * count)(*[spng.ChunkingDesc(data.data_ptr() + i * length, length, dst.data_ptr() + i * cap, cap, chunk_bytes)
                                             for i in range(count)])
        res = s.empty(count * ctypes.sizeof(spng.Result))
        return dst, cap, lambda: spng._check(s.lib, s.lib.spng_write_idat_batch(s.ctx, arr, count, res.data_ptr(), None))

    def files(count, length, chunk_bytes, on_device):
        d, k = spng.png_desc((4096, 4096), 8, 4, chunk_bytes=chunk_bytes)
        cap = int(s.lib.spng_file_bound(ctypes.byref(d), length))
        dst = s.empty(count * cap)
        src_res = None
        if on_device:
            rec = bytes(spng.Result(0, 0, length, 0, (ctypes.c_uint64 * 2)(0, 0)))
            src_res = s.to_device(rec * count)
        arr = (spng.PngDesc * count)()
        for i in range(count):
            d, k2 = spng.png_desc((4096, 4096), 8, 4, chunk_bytes=chunk_bytes)
            d.d_stream, d.stream_len, d.stream_cap = data.data_ptr() + i * length, 0 if on_device else length, length
            d.d_stream_result = src_res.data_ptr() + i * ctypes.sizeof(spng.Result) if on_device else None
            d.d_out, d.out_cap = dst.data_ptr() + i * cap, cap
            arr[i] = d
        res = s.empty(count * ctypes.sizeof(spng.Result))
        return dst, cap, (res, src_res), lambda: spng._check(s.lib, s.lib.spng_write_file_batch(s.ctx, arr, count, res.data_ptr(), None))

    for label, count, length, chunk_bytes, old_steps in (("many", n, each, CHUNK, steps), ("one", 1, total, 0x7fffffff, max(a.old_one_steps, 1))):
        old_dst, old_cap, old = chunking(count, length, chunk_bytes)
        new_dst, new_cap, keep1, new = files(count, length, chunk_bytes, False)
        dev_dst, _, keep2, dev = files(count, length, chunk_bytes, True)
        r = {"chunk_bytes": chunk_bytes, "idat_chunks": count * -(-length // chunk_bytes)}
        r["write_idat_ms"], r["write_idat_min"], r["write_idat_max"] = timed(s, spng, old, old_steps, 1 if label == "one" else a.warmup)
        r["write_idat_steps"] = old_steps
        r["write_file_ms"], r["write_file_min"], r["write_file_max"] = timed(s, spng, new, steps, a.warmup)
        r["write_file_device_len_ms"], r["write_file_device_len_min"], r["write_file_device_len_max"] = timed(s, spng, dev, steps, a.warmup)
        r["write_file_gbps"] = round(2 * count * length / (r["write_file_ms"] * 1e-3) / 1e9, 1)
        r["ratio_old_over_new"] = round(r["write_idat_ms"] / r["write_file_ms"], 3)
        # after the clock: the chunks of both writers are the same bytes, and the device-length form wrote the same files
        for i in (0, count - 1):
            a0 = new_dst[i * new_cap + 8 + head:i * new_cap + 8 + head + old_cap]
            assert torch.equal(a0, old_dst[i * old_cap:(i + 1) * old_cap]), (label, i)
        assert torch.equal(new_dst, dev_dst), label
        res = (spng.Result * count).from_buffer_copy(bytes(keep1[0].cpu().numpy()))
        assert all(x.status == 0 and x.written == new_cap and x.consumed == length for x in res), label
        out[label] = r
        del old_dst, new_dst, dev_dst
    dst = s.empty(total)
    ms = ctypes.c_double(0)
    spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, dst.data_ptr(), data.data_ptr(), total, 0, max(steps, 5), ctypes.byref(ms)))
    out["copy_ceiling_ms"] = round(ms.value, 4)
    out["copy_ceiling_gbps"] = round(2 * total / (ms.value * 1e-3) / 1e9, 1)
    out["one_over_many"] = round(out["one"]["write_file_ms"] / out["many"]["write_file_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
