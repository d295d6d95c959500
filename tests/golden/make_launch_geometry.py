#!/usr/bin/env python3
"""Regenerates tests/golden/launch_geometry.json: inputs and outputs of the launch arithmetic (swift_png_amd/csrc/geometry.hpp),
about two hundred rows per function, which tests/test_launch_geometry.py holds the library's functions to.

The inputs are made here (the case table of tests/scanline_cases.py, the edges of every threshold, seeded sweeps); the outputs are
whatever tests/scanline_cases.py `unfilter_plan` and tests/geometry.py answer in the tree this runs in.  The committed file was
written by this script in the tree BEFORE the arithmetic moved into geometry.hpp -- `unfilter_plan` was a restatement in Python
then, and a stand-in for tests/geometry.py called the function bodies as they stood in csrc/api.hip -- so it pins what the host
layer computed when it was written inline; run in a later tree it must write the same bytes."""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import geometry as geo          # noqa: E402
import scanline_cases as sc     # noqa: E402


def log_uniform(rng, lo, hi, n):
    return [int(x) for x in np.exp(rng.uniform(np.log(lo), np.log(hi + 1), n)).astype(np.uint64).clip(lo, hi)]


def around(*marks):
    return sorted({m + d for m in marks for d in (-1, 0, 1) if m + d >= 0})


def unfilter_rows():
    calls = []                                                  # (k, jobs [(pitch, rows)], configured)
    seen = set()
    for c in sc.PRIMARY + sc.SECONDARY + sc.ADAM7_CASES + sc.RESUME_CASES:
        if c.fmt not in seen:
            seen.add(c.fmt)
            calls.append((c.bpp, [(p, h) for p, h, _ in sc.passes(c)], 0))
    for c in sc.KNOB_CASES:
        calls += [(c.bpp, [(p, h) for p, h, _ in sc.passes(c)], v) for v in sc.KNOB_VALUES]
    batches = [(k, sc.batch_cases(k)) for k in sorted(sc.BATCH_FORMATS)]
    batches += [(1, sc.scaled_batch_cases()), (1, sc.wide_batch_cases(False)), (1, sc.wide_batch_cases(True))]
    batches += [(k, sc.floor4_batch_cases(k)) for k in (4, 8)]
    calls += [(k, [(p, h) for c in cases for p, h, _ in sc.passes(c)], 0) for k, cases in batches]
    rng = np.random.default_rng(0x9e0)
    for i in range(200):                                        # k in {1, 2, 3, 4, 6, 8}, 1 .. 400 jobs, pitches 1 .. 70 000, rows 1 .. 9 000
        k = (1, 2, 3, 4, 6, 8)[i % 6]
        n, pmax, rmax = int(rng.integers(1, 401)), log_uniform(rng, 1, 70000, 1)[0], log_uniform(rng, 16, 9000, 1)[0]
        calls.append((k, list(zip(rng.integers(1, pmax + 1, n).tolist(), rng.integers(1, rmax + 1, n).tolist())), 0))
    out = []
    for k, jobs, configured in calls:
        kernel, rule, piece, pieces = sc.unfilter_plan(k, jobs, configured)
        out.append([k, sum(r for _, r in jobs), max(r for _, r in jobs), max(p for p, _ in jobs), configured, kernel, rule, piece, pieces])
    return out


def main():
    rng = np.random.default_rng(0x9e1)
    table = {"unfilter_pieces": unfilter_rows()}                # [k, total rows, max rows, widest, configured, kernel, rule, piece rows, pieces]
    rows = around(1, 4, 4 * 4096, 8 * 4096, (1 << 32) - 2) + log_uniform(rng, 1, 1 << 31, 170)
    table["filter_blocks_x"] = [[r, geo.filter_blocks_x(r)] for r in rows]
    pix = around(1, 256, 512, 256 * 1024, 256 * 4096, 1 << 31) + log_uniform(rng, 1, 1 << 36, 80)
    table["plane_blocks_x"] = [[p, cap, geo.plane_blocks_x(p, cap)] for cap in (1024, 4096) for p in pix]
    most = around(1, 4096, 16384, 4096 * 4096, 16384 * 4096, 1 << 32) + log_uniform(rng, 1, 1 << 40, 80)
    table["blocks_for"] = [[m, per, geo.blocks_for(m, per)] for per in (4096, 16384) for m in most]
    counts = around(2, 16, 256, 4096, 65536) + log_uniform(rng, 1, 1 << 20, 15)
    table["census_blocks_x"] = [[c, m, geo.census_blocks_x(c, m)] for c in counts for m in (1, 1024, 1025, 16 * 1024, 16 * 1024 + 1, 100000, 1 << 22, 1 << 34)]
    pieces = around(1, 4096, 1 << 32) + log_uniform(rng, 1, 1 << 40, 190)
    table["write_idat_blocks_x"] = [[m, geo.write_idat_blocks_x(m)] for m in pieces]
    lens = around(1, 12, 24, 756, 768, 2048, 2048 * (8192 - 64), 1 << 32) + log_uniform(rng, 1, 1 << 34, 180)
    table["lex_listed"] = [[n, geo.lex_listed(n)] for n in lens]
    totals = around(1, 64 << 10, 4096 * (32 << 10), 4096 * (64 << 10), 4096 * (256 << 10), 32768 * (256 << 10), 10 << 30) + log_uniform(rng, 1, 1 << 40, 20)
    table["inflate_segment_bytes"] = [[0, t, b, geo.inflate_segment_bytes(0, t, b)] for b in (0.0, 1.0, 2047.5, 8191.5, 8192.0, 40000.0) for t in totals]
    table["inflate_segment_bytes"] += [[c, t, b, geo.inflate_segment_bytes(c, t, b)] for c in (1, 255, 256, 257, 65536, (1 << 20) + 1) for t in (1, 1 << 30)
                                       for b in (0.0, 2047.5)]
    streams = list(range(1, 140)) + around(255, 256, 257, 65536) + log_uniform(rng, 1, 1 << 30, 50)
    table["search_chunks"] = [[s, *geo.search_chunks(s)] for s in streams]
    with open(HERE / "launch_geometry.json", "w") as f:
        f.write("{\n" + ",\n".join(f'"{name}": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]" for name, rows in table.items()) + "\n}\n")
    print({name: len(rows) for name, rows in table.items()})


if __name__ == "__main__":
    main()
