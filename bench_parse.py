"""bench_parse.py -- the typed chunks on the device (spng_parse_dir_batch) beside the directory they ride on.  One JSON line per section.

    small   the `lex` shape of bench_metadata.py -- the 28 baseline files of tests/golden/encode replicated to 8192, resident in HBM --:
            spng_lex_dir_batch, then spng_parse_dir_batch over what it left on the device, a step of one then a step of the other.  With
            --parent-lib, a build of the parent commit is loaded beside this one and its spng_lex_dir_batch takes turns with them: "has the
            directory moved" within one process.  Per entry: the call on the host clock, from an idle stream to an idle stream, and its
            kernels by the profile timer (SPNG_K_LEX: device events around the call's launches); median, min, max of the steps.
    splt    one file with one sPLT of --splt-mib MiB (entries of 6 bytes, equal frequencies: the whole chunk is walked) on the single wave
            that parses it.

    python bench_parse.py [--steps 11] [--warmup 2] [--files 8192] [--splt-mib 64] [--parent-lib PATH] [--parent-first] [--only small,splt]"""
from __future__ import annotations

import argparse
import ctypes
import json
import struct
import time
import zlib
from pathlib import Path

from bench_metadata import raw_library, spread

ROOT = Path(__file__).resolve().parent


def timed(lib, ctx, spng, call):
    """-> (host ms from an idle stream to an idle stream, ms of the call's kernels)"""
    lib.spng_sync(ctx)
    lib.spng_profile(ctx, 1)
    t0 = time.perf_counter()
    assert call() == 0
    lib.spng_sync(ctx)
    dt = time.perf_counter() - t0
    ms, launches = ctypes.c_double(0), ctypes.c_uint64(0)
    assert lib.spng_profile_get(ctx, spng.K_LEX, ctypes.byref(ms), ctypes.byref(launches)) == 0
    return dt * 1e3, ms.value


def section_small(a, torch, spng, s):
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
    esz, vsz = ctypes.sizeof(spng.ChunkEntry), ctypes.sizeof(spng.ChunkValue)
    d_ent = torch.empty(sum(caps) * esz, dtype=torch.uint8, device=s.tdev)
    d_val = torch.empty(sum(caps) * vsz, dtype=torch.uint8, device=s.tdev)
    d_infos = torch.empty(n * ctypes.sizeof(spng.Lexed), dtype=torch.uint8, device=s.tdev)
    d_parsed = torch.empty(n * ctypes.sizeof(spng.Parsed), dtype=torch.uint8, device=s.tdev)
    at, dirs, vals = 0, (spng.ChunkDir * n)(), (ctypes.c_void_p * n)()
    for j in range(n):
        dirs[j] = spng.ChunkDir(d_ent.data_ptr() + at * esz, caps[j], 0)
        vals[j] = d_val.data_ptr() + at * vsz
        at += caps[j]
    entries = {"lex_dir": (s.lib, s.ctx, lambda: s.lib.spng_lex_dir_batch(s.ctx, fdescs, dirs, n, d_infos.data_ptr(), None)),
               "parse_dir": (s.lib, s.ctx, lambda: s.lib.spng_parse_dir_batch(s.ctx, fdescs, dirs, d_infos.data_ptr(), vals, n, d_parsed.data_ptr(), None))}
    if a.parent_lib:
        plib, pctx = raw_library(a.parent_lib, spng)
        plib.spng_lex_dir_batch.argtypes = s.lib.spng_lex_dir_batch.argtypes
        entries["parent_lex_dir"] = (plib, pctx, lambda: plib.spng_lex_dir_batch(pctx, fdescs, dirs, n, d_infos.data_ptr(), None))
        if a.parent_first:                                       # (the turn a call takes within a step is a variable of its own)
            entries = {k: entries[k] for k in ("parent_lex_dir", "lex_dir", "parse_dir")}
    host = {k: [] for k in entries}
    kern = {k: [] for k in entries}
    for step in range(a.warmup + a.steps):
        for k, (lib, ctx, call) in entries.items():
            dt, ms = timed(lib, ctx, spng, call)
            if step >= a.warmup:
                host[k].append(dt)
                kern[k].append(ms)
    parsed = (spng.Parsed * n).from_buffer_copy(d_parsed.cpu().numpy().tobytes())
    infos = (spng.Lexed * n).from_buffer_copy(d_infos.cpu().numpy().tobytes())
    assert all(p.status == 0 and p.ihdr_index == 0 for p in parsed) and all(r.status == 0 for r in infos)
    out = {"section": "small", "files": n, "file_bytes": sum(len(files[j % 28]) for j in range(n)), "steps": a.steps, "warmup": a.warmup,
           "chunks": sum(r.chunks for r in infos), "order": list(entries)}
    for k in entries:
        out[k] = {"host": spread(host[k]), "kernels": spread(kern[k])}
    print(json.dumps(out), flush=True)


def section_splt(a, torch, spng, s):
    entries = (a.splt_mib << 20) // 6
    payload = b"p\0\x08" + (b"\x11\x22\x33\x44" + struct.pack(">H", 7)) * entries
    chunk = lambda name, data: struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data))  # noqa: E731
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 1, 1, 8, 0, 0, 0, 0)) + chunk(b"sPLT", payload) + chunk(b"IEND", b"")
    d_png = s.to_device(data)
    d_ent, d_val = s.empty(4 * ctypes.sizeof(spng.ChunkEntry)), s.empty(4 * ctypes.sizeof(spng.ChunkValue))
    d_infos, d_parsed = s.empty(ctypes.sizeof(spng.Lexed)), s.empty(ctypes.sizeof(spng.Parsed))
    fdescs = (spng.FileDesc * 1)(spng.FileDesc(d_png.data_ptr(), len(data), None, 0))
    dirs = (spng.ChunkDir * 1)(spng.ChunkDir(d_ent.data_ptr(), 4, 0))
    vals = (ctypes.c_void_p * 1)(d_val.data_ptr())
    assert s.lib.spng_lex_dir_batch(s.ctx, fdescs, dirs, 1, d_infos.data_ptr(), None) == 0
    host, kern = [], []
    for step in range(a.splt_warmup + a.splt_steps):
        dt, ms = timed(s.lib, s.ctx, spng, lambda: s.lib.spng_parse_dir_batch(s.ctx, fdescs, dirs, d_infos.data_ptr(), vals, 1, d_parsed.data_ptr(), None))
        if step >= a.splt_warmup:
            host.append(dt)
            kern.append(ms)
    value = (spng.ChunkValue * 4).from_buffer_copy(d_val.cpu().numpy().tobytes())[1]
    assert (value.status, value.scope, value.count, value.k, value.v[0]) == (0, spng.SCOPE_PARSED, entries, 1, 8)
    print(json.dumps({"section": "splt", "payload_bytes": len(payload), "entries": entries, "steps": a.splt_steps, "warmup": a.splt_warmup,
                      "host": spread(host), "kernels": spread(kern),
                      "gbps": round(len(payload) / (sorted(kern)[len(kern) // 2] * 1e-3) / 1e9, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--splt-mib", type=int, default=64)
    ap.add_argument("--splt-steps", type=int, default=3)
    ap.add_argument("--splt-warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="small: the parent's call takes the first turn of every step, not the last")
    ap.add_argument("--only", default="small,splt")
    a = ap.parse_args()
    import torch
    import swift_png_amd as spng
    s = spng.load(0)
    for name in a.only.split(","):
        {"small": section_small, "splt": section_splt}[name](a, torch, spng, s)


if __name__ == "__main__":
    main()
