"""bench_metadata.py -- the metadata path on the device: the chunk directory beside the lexer it rides on, the text entry beside the
library's copy ceiling, and the ImageMetadata round trip stage by stage.  One JSON line per section, printed as it finishes.

    lex         spng_lex_batch over the `small_images` shape of bench.py -- the 28 baseline files of tests/golden/encode replicated to 8192,
                resident in HBM -- and spng_lex_dir_batch over the same files, a step of one then a step of the other.  With
                --parent-lib, a build of the parent commit is loaded beside this one and its spng_lex_batch takes turns with them: the
                comparison "has the lexer moved" within one process.  Per entry: the call on the host clock (it ends in a wait for the
                infos) and its kernels by the profile timer (SPNG_K_LEX); median, min, max of the steps.
    text        spng_text_batch over 256 MiB of text of which every second byte is >= 0x80: transcoded, then the result checked;
                bytes read and written over kernel time, as a fraction of spng_copy_ceiling on the same buffer in the same process.
    round_trip  `--copies` copies of tests/golden/metadata/ImageMetadata.png: lex + directory, inflate (the zTXt and the iCCP body of every
                file), transcode (Latin-1 -> UTF-8), deflate (level 13, the text and the profile of every file), write (signature,
                head with the new chunks, the file's IDAT stream, IEND); each stage's library call on the host clock, from an idle stream to an
                idle stream (building the descriptors is not in it).

    python bench_metadata.py [--steps 11] [--warmup 2] [--copies 1024] [--text-mib 256] [--parent-lib PATH] [--only lex,text,round_trip]"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import struct
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def raw_library(path, spng):
    """a build of the library by its path, with the few prototypes the lexer's clock needs (a parent build lacks this commit's exports)"""
    lib = ctypes.CDLL(str(path))
    vp = ctypes.c_void_p
    lib.spng_create.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
    lib.spng_lex_batch.argtypes = [vp, ctypes.POINTER(spng.FileDesc), ctypes.c_uint32, vp, ctypes.POINTER(spng.Lexed)]
    lib.spng_profile.argtypes = [vp, ctypes.c_int]
    lib.spng_profile_get.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    lib.spng_sync.argtypes = [vp]
    ctx = vp()
    assert lib.spng_create(0, None, ctypes.byref(ctx)) == 0
    return lib, ctx


def section_lex(a, torch, spng, s):
    files = [p.read_bytes() for p in sorted((ROOT / "tests" / "golden" / "encode").glob("*.baseline.png"))]
    assert len(files) == 28
    n = a.files
    d_files = [s.to_device(f) for f in files]
    al = lambda v: (v + 255) & ~255                              # noqa: E731
    offs = [0]
    for j in range(n):
        offs.append(offs[-1] + al(len(files[j % 28])))
    d_idat = torch.empty(offs[-1], dtype=torch.uint8, device=s.tdev)
    fdescs = (spng.FileDesc * n)(*[spng.FileDesc(d_files[j % 28].data_ptr(), len(files[j % 28]), d_idat.data_ptr() + offs[j], al(len(files[j % 28])))
                                   for j in range(n)])
    caps = [len(files[j % 28]) // 12 for j in range(n)]
    size = ctypes.sizeof(spng.ChunkEntry)
    d_ent = torch.empty(sum(caps) * size, dtype=torch.uint8, device=s.tdev)
    at, dirs = 0, (spng.ChunkDir * n)()
    for j in range(n):
        dirs[j] = spng.ChunkDir(d_ent.data_ptr() + at * size, caps[j], 0)
        at += caps[j]
    infos = {k: (spng.Lexed * n)() for k in ("lex", "lex_dir", "parent_lex")}
    entries = {"lex": (s.lib, s.ctx, lambda: s.lib.spng_lex_batch(s.ctx, fdescs, n, None, infos["lex"])),
               "lex_dir": (s.lib, s.ctx, lambda: s.lib.spng_lex_dir_batch(s.ctx, fdescs, dirs, n, None, infos["lex_dir"]))}
    if a.parent_lib:
        plib, pctx = raw_library(a.parent_lib, spng)
        entries["parent_lex"] = (plib, pctx, lambda: plib.spng_lex_batch(pctx, fdescs, n, None, infos["parent_lex"]))
    host = {k: [] for k in entries}
    kern = {k: [] for k in entries}
    for step in range(a.warmup + a.steps):
        for k, (lib, ctx, call) in entries.items():
            lib.spng_profile(ctx, 1)
            t0 = time.perf_counter()
            assert call() == 0
            dt = time.perf_counter() - t0
            ms, launches = ctypes.c_double(0), ctypes.c_uint64(0)
            assert lib.spng_profile_get(ctx, spng.K_LEX, ctypes.byref(ms), ctypes.byref(launches)) == 0
            if step >= a.warmup:
                host[k].append(dt * 1e3)
                kern[k].append(ms.value)
    assert all(r.status == 0 for r in infos["lex"]) and all(bytes(v) == bytes(infos["lex"]) for v in infos.values() if v[0].width)
    out = {"section": "lex", "files": n, "file_bytes": sum(len(files[j % 28]) for j in range(n)), "steps": a.steps, "warmup": a.warmup,
           "chunks": sum(r.chunks for r in infos["lex"])}
    for k in entries:
        out[k] = {"host": spread(host[k]), "kernels": spread(kern[k])}
    print(json.dumps(out), flush=True)


def section_text(a, torch, spng, s):
    n = a.text_mib << 20
    g = torch.Generator(device=s.tdev).manual_seed(16)
    data = torch.randint(0x20, 0x7f, (n,), dtype=torch.uint8, device=s.tdev, generator=g)
    data[::2] |= 0x80                                           # every second byte >= 0x80
    dst = s.empty(2 * n)
    res = s.empty(2 * ctypes.sizeof(spng.Result))
    zero = (ctypes.c_uint8 * 7)()
    transcode = (spng.TextDesc * 1)(spng.TextDesc(data.data_ptr(), n, dst.data_ptr(), 2 * n, spng.TEXT_LATIN1_TO_UTF8, zero))
    check = (spng.TextDesc * 1)(spng.TextDesc(dst.data_ptr(), n + n // 2, None, 0, spng.TEXT_CHECK_UTF8, zero))
    out = {"section": "text", "bytes": n, "high_bytes": n // 2, "steps": a.steps, "warmup": a.warmup}
    for name, descs, moved in (("transcode", transcode, 2 * n + n + n // 2), ("check_utf8", check, n + n // 2)):
        ms = []
        for step in range(a.warmup + a.steps):
            s.profile(True)
            spng._check(s.lib, s.lib.spng_text_batch(s.ctx, descs, 1, res.data_ptr(), None))
            s.sync()
            if step >= a.warmup:
                ms.append(s.profile_get(spng.K_LEX)[0])
        s.profile(False)
        r = spng.Result.from_buffer_copy(bytes(res[:ctypes.sizeof(spng.Result)].cpu().numpy()))
        assert r.status == 0 and r.written == (n + n // 2 if name == "transcode" else 0), (name, r.status, r.written)
        out[name] = dict(spread(ms), bytes_moved=moved, gbps=round(moved / (statistics.median(ms) * 1e-3) / 1e9, 1))
    ms = ctypes.c_double(0)
    spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, dst.data_ptr(), data.data_ptr(), n, 0, max(a.steps, 5), ctypes.byref(ms)))
    out["copy_ceiling_ms"] = round(ms.value, 4)
    out["copy_ceiling_gbps"] = round(2 * n / (ms.value * 1e-3) / 1e9, 1)
    for name in ("transcode", "check_utf8"):
        out[name]["fraction_of_copy_ceiling"] = round(out[name]["gbps"] / out["copy_ceiling_gbps"], 3)
    print(json.dumps(out), flush=True)


def clocked(s, spng, call):
    """the library call alone on the host clock, from an idle stream to an idle stream: -> ms"""
    s.sync()
    t0 = time.perf_counter()
    spng._check(s.lib, call())
    s.sync()
    return (time.perf_counter() - t0) * 1e3


def section_round_trip(a, torch, spng, s):
    data = (ROOT / "tests" / "golden" / "metadata" / "ImageMetadata.png").read_bytes()
    n = a.copies
    d_png = s.to_device(data)                                    # (the copies read the same bytes; every output is a file's own)
    d_idat = torch.empty(n * len(data), dtype=torch.uint8, device=s.tdev)
    fdescs = (spng.FileDesc * n)(*[spng.FileDesc(d_png.data_ptr(), len(data), d_idat.data_ptr() + j * len(data), len(data)) for j in range(n)])
    cap = 16
    size = ctypes.sizeof(spng.ChunkEntry)
    d_ent = torch.empty(n * cap * size, dtype=torch.uint8, device=s.tdev)
    dirs = (spng.ChunkDir * n)(*[spng.ChunkDir(d_ent.data_ptr() + j * cap * size, cap, 0) for j in range(n)])
    infos = (spng.Lexed * n)()
    state = {}

    def lex():
        ms = clocked(s, spng, lambda: s.lib.spng_lex_dir_batch(s.ctx, fdescs, dirs, n, None, infos))
        state["entries"] = (spng.ChunkEntry * (n * cap)).from_buffer_copy(bytes(d_ent.cpu().numpy()))
        return ms

    def inflate():
        e = state["entries"]
        picks = [(j, e[j * cap + c]) for j in range(n) for c in range(min(infos[j].chunks, cap)) if e[j * cap + c].compressed]
        caps = [1 << 16 if x.length > 1000 else 1 << 12 for _, x in picks]
        if "inflated" not in state:
            state["inflated"] = [s.empty(c) for c in caps]
        descs = (spng.StreamDesc * len(picks))(*[spng.StreamDesc(d_png.data_ptr() + x.offset + x.body_off, x.length - x.body_off, o.data_ptr(), c, 0, 0)
                                                 for (_, x), o, c in zip(picks, state["inflated"], caps)])
        res = (spng.Result * len(picks))()
        ms = clocked(s, spng, lambda: s.lib.spng_inflate_batch(s.ctx, descs, len(picks), None, res))
        assert all(r.status == 0 for r in res)
        state["picks"], state["lens"] = picks, [r.written for r in res]
        return ms

    def transcode():
        texts = [k for k, (_, x) in enumerate(state["picks"]) if struct.pack(">I", x.type) != b"iCCP"]
        if "utf8" not in state:
            state["utf8"] = [s.empty(2 * state["lens"][k]) for k in texts]
        descs = (spng.TextDesc * len(texts))(*[spng.TextDesc(state["inflated"][k].data_ptr(), state["lens"][k], o.data_ptr(), o.numel(),
                                                             spng.TEXT_LATIN1_TO_UTF8, (ctypes.c_uint8 * 7)()) for k, o in zip(texts, state["utf8"])])
        res = (spng.Result * len(texts))()
        ms = clocked(s, spng, lambda: s.lib.spng_text_batch(s.ctx, descs, len(texts), None, res))
        assert all(r.status == 0 for r in res)
        state["texts"], state["utf8_lens"] = texts, [r.written for r in res]
        return ms

    def deflate():
        srcs = [(o, m) for o, m in zip(state["utf8"], state["utf8_lens"])]
        srcs += [(state["inflated"][k], state["lens"][k]) for k in range(len(state["picks"])) if k not in state["texts"]]
        if "deflated" not in state:
            state["deflated"] = [s.empty(int(s.lib.spng_deflate_bound(m))) for _, m in srcs]
        descs = (spng.StreamDesc * len(srcs))(*[spng.StreamDesc(o.data_ptr(), m, d.data_ptr(), d.numel(), 0, 0) for (o, m), d in zip(srcs, state["deflated"])])
        levels = (ctypes.c_int32 * len(srcs))(*([13] * len(srcs)))
        res = (spng.Result * len(srcs))()
        ms = clocked(s, spng, lambda: s.lib.spng_deflate_batch(s.ctx, descs, levels, len(srcs), None, res))
        assert all(r.status == 0 for r in res)
        state["deflated_lens"] = [r.written for r in res]
        return ms

    def write():
        # the finished blobs come to the host (the writer takes them from there), the IDAT stream stays where the lexer put it
        first = (0, len(state["texts"]))                         # (the first text, the first profile: the copies' are the same bytes)
        blobs = [bytes(state["deflated"][k][:state["deflated_lens"][k]].cpu().numpy()) for k in first]
        text = b"Raw profile type exif\0\1\0en\0\0" + blobs[0]
        profile = b"ICC profile\0\0" + blobs[1]
        arr, keep, outs = (spng.PngDesc * n)(), [], state.setdefault("files", [])
        for j in range(n):
            d, k = spng.png_desc((infos[j].width, infos[j].height), 8, 4, fill=(255, 255, 255), before=[(b"iCCP", profile)], after=[(b"iTXt", text)])
            d.d_stream, d.stream_len, d.stream_cap = d_idat.data_ptr() + j * len(data), infos[j].idat_len, infos[j].idat_len
            if len(outs) <= j:
                outs.append(s.empty(int(s.lib.spng_file_bound(ctypes.byref(d), infos[j].idat_len))))
            d.d_out, d.out_cap = outs[j].data_ptr(), outs[j].numel()
            arr[j] = d
            keep.append(k)
        res = (spng.Result * n)()
        ms = clocked(s, spng, lambda: s.lib.spng_write_file_batch(s.ctx, arr, n, None, res))
        assert all(r.status == 0 for r in res)
        return ms

    stages = (("lex_dir", lex), ("inflate", inflate), ("transcode", transcode), ("deflate", deflate), ("write", write))
    ms = {k: [] for k, _ in stages}
    for step in range(a.warmup + a.steps):
        for k, stage in stages:
            t = stage()
            if step >= a.warmup:
                ms[k].append(t)
    out = {"section": "round_trip", "copies": n, "file_bytes": len(data), "steps": a.steps, "warmup": a.warmup,
           "inflate_streams": len(state["picks"]), "deflate_streams": len(state["deflated"]), "text_bytes": state["lens"][0],
           "deflated_text_bytes": state["deflated_lens"][0]}
    for k, _ in stages:
        out[k] = spread(ms[k])
    out["total_median_ms"] = round(sum(out[k]["median_ms"] for k, _ in stages), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--copies", type=int, default=1024)
    ap.add_argument("--text-mib", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="lex,text,round_trip")
    a = ap.parse_args()
    import torch
    import swift_png_amd as spng
    s = spng.load(0)
    for name in a.only.split(","):
        {"lex": section_lex, "text": section_text, "round_trip": section_round_trip}[name](a, torch, spng, s)


if __name__ == "__main__":
    main()
