"""Times spng_census_wide_batch and spng_map_batch against the old entries and the copy ceiling measured in the same process
(profiles/r13_colour_tables.md):

    python tools/probe_colour_tables.py [--side 4096] [--runs 7] [--out FILE]

(a) the CustomColor tutorial's picture (tests/golden/customcolor/CustomColor.png: 235 200 pixels, 97 388 keys): wide census, 8-byte map;
(b) a side^2 RGBA8 raster of 60 000 colours: spng_census_batch beside spng_census_wide_batch, and spng_pack_indexed_batch beside
    spng_map_batch with 1-byte values, on the same input -- the comparison with what the library did before;
(c) a side^2 raster of uniformly random RGBA8 (nearly side^2 keys): wide census, 4-byte map, the scratch taken, the sort's launches.
Kernel time comes from spng_profile (HIP events around the launches of a call; for the wide census that is the counting stage plus the
stages behind the call's one wait, not the wait itself), one call per reading after a first, untimed call; median and min - max of
`runs` readings.  GB/s counts the bytes an entry must move (pixels in; keys and counts, or values, out); `of ceiling` is that over
spng_copy_ceiling pattern 0 on 2 x 128 MiB in the same run.  Prints a markdown table."""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import swift_png_amd as spng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 5
    import numpy as np
    import torch
    import pnghelp as ph
    s = spng.load(0)
    half = 128 << 20
    a, b = torch.zeros(half, dtype=torch.uint8, device=s.tdev), torch.empty(half, dtype=torch.uint8, device=s.tdev)
    ms = ctypes.c_double(0)
    spng._check(s.lib, s.lib.spng_copy_ceiling(s.ctx, b.data_ptr(), a.data_ptr(), half, 0, args.runs, ctypes.byref(ms)))
    ceiling = 2 * half / (ms.value * 1e-3) / 1e9
    del a, b
    torch.cuda.empty_cache()
    lines = [f"library {spng.LIB_PATH.name}, source digest {spng.source_digest()}, {args.runs} readings of one call each after a first call; "
             f"copy ceiling (pattern 0, 2 x 128 MiB) {ceiling:.0f} GB/s", "",
             "| input | entry | keys | ms median | min - max | GB/s | of ceiling | note |", "|---|---|---|---|---|---|---|---|"]

    def timed(kernel, call):
        call()                                                  # first touch: scratch grown, code loaded
        s.sync()
        readings = []
        for _ in range(args.runs):
            s.profile(True)
            call()
            t, _ = s.profile_get(kernel)
            s.profile(False)
            readings.append(t)
        return statistics.median(readings), min(readings), max(readings)

    def row(what, entry, keys, t, nbytes, note=""):
        rate = nbytes / (t[0] * 1e-3) / 1e9
        lines.append(f"| {what} | {entry} | {keys} | {t[0]:.3f} | {t[1]:.3f} - {t[2]:.3f} | {rate:.1f} | {rate / ceiling:.3f} | {note} |")
        return t[0]

    def keys_of(d_px, n, cap):
        ((k, c),), (r,) = s.census_wide_batch([d_px], 8, 0, cap=cap)
        assert r.status == 0
        return k[:r.written], int(r.written)

    # (a) the tutorial's picture
    png = ph.parse_png((ROOT / "tests" / "golden" / "customcolor" / "CustomColor.png").read_bytes())
    st, storage, _ = s.decode(png.idat, png.width, png.height, 8, 3, False)
    assert st == 0
    rgb = np.frombuffer(storage, dtype=np.uint8).reshape(-1, 3)
    rgba = np.concatenate([rgb, np.full((len(rgb), 1), 255, dtype=np.uint8)], axis=1)
    n = len(rgba)
    d_px = s.to_device(rgba.tobytes())
    d_keys, nk = keys_of(d_px, n, n)
    outs = [(torch.empty(n, dtype=torch.int32, device=s.tdev), torch.empty(n, dtype=torch.int64, device=s.tdev))]
    t = timed(spng.K_CENSUS, lambda: s.census_wide_batch([d_px], 8, 0, cap=n, outs=outs))
    row(f"CustomColor, {n} px", "census_wide", nk, t, 4 * n + 12 * nk, f"{spng.census_wide_sort_launches(nk)} sort launches")
    d_val, d_out = torch.zeros(8 * nk, dtype=torch.uint8, device=s.tdev), s.empty(8 * n)
    t = timed(spng.K_PACK_INDEXED, lambda: s.map_batch([d_px], 8, 0, [d_keys], [d_val], 8, outs=[d_out]))
    row(f"CustomColor, {n} px", "map, 8-byte values", nk, t, 12 * n)

    # (b) 60 000 colours: the old entries beside the new ones
    n = args.side * args.side
    rng = np.random.default_rng(13)
    colours = np.unique(rng.integers(0, 1 << 32, 70000, dtype=np.uint64).astype(np.uint32))[:60000]
    px = rng.permutation(colours)[rng.integers(0, 60000, n)]
    px[:60000] = colours
    d_px = s.to_device(px.view(np.uint8))
    what = f"{args.side}^2, 60 000 colours"
    old_outs = [(torch.empty(65536, dtype=torch.int32, device=s.tdev), torch.empty(65536, dtype=torch.int64, device=s.tdev))]
    t_old = row(what, "census (old)", 60000, timed(spng.K_CENSUS, lambda: s.census_batch([d_px], 8, 0, 65536, outs=old_outs)), 4 * n + 12 * 60000)
    t_new = row(what, "census_wide", 60000, timed(spng.K_CENSUS, lambda: s.census_wide_batch([d_px], 8, 0, cap=65536, outs=old_outs)),
                4 * n + 12 * 60000, f"{spng.census_wide_sort_launches(60000)} sort launches")
    lines[-1] = lines[-1][:-2] + f"; {t_new / t_old:.2f} x the old entry's time |"
    d_keys = old_outs[0][0][:60000].clone()
    assert (d_keys.cpu().numpy().view(np.uint32) == colours).all()
    d_idx, d_out = torch.randint(0, 256, (60000,), dtype=torch.uint8, device=s.tdev), s.empty(n)
    t_old = row(what, "pack_indexed (old)", 60000,
                timed(spng.K_PACK_INDEXED, lambda: s.pack_indexed_batch([d_px], [(args.side, args.side)], 8, 0, [d_keys], [d_idx], storages=[d_out])), 5 * n)
    first = d_out.clone()
    t_new = row(what, "map, 1-byte values", 60000, timed(spng.K_PACK_INDEXED, lambda: s.map_batch([d_px], 8, 0, [d_keys], [d_idx], 1, outs=[d_out])), 5 * n)
    lines[-1] = lines[-1][:-2] + f"{t_new / t_old:.2f} x the old entry's time |"
    assert bool((first == d_out).all())

    # (c) random RGBA8: nearly side^2 keys
    del d_px
    s.trim()
    torch.cuda.empty_cache()
    d_px = torch.randint(0, 256, (4 * n,), dtype=torch.uint8, device=s.tdev)
    cap = min(n, spng.CENSUS_WIDE_CAP)
    d_keys, nk = keys_of(d_px, n, cap)
    pow2 = 1 << (cap - 1).bit_length()
    scratch = 256 + 16 * max(64, 2 * pow2) + 8 * pow2             # the header's formula: the table of 2 cap slots, the sort buffer
    outs = [(torch.empty(cap, dtype=torch.int32, device=s.tdev), torch.empty(cap, dtype=torch.int64, device=s.tdev))]
    what = f"{args.side}^2, random"
    t = timed(spng.K_CENSUS, lambda: s.census_wide_batch([d_px], 8, 0, cap=cap, outs=outs))
    row(what, "census_wide", nk, t, 4 * n + 12 * nk, f"{spng.census_wide_sort_launches(nk)} sort launches, {scratch / 2 ** 20:.0f} MiB of scratch")
    d_keys = outs[0][0][:nk]
    d_val, d_out = torch.zeros(4 * nk, dtype=torch.uint8, device=s.tdev), s.empty(4 * n)
    slots = 64
    while slots < 2 * nk:
        slots *= 2
    t = timed(spng.K_PACK_INDEXED, lambda: s.map_batch([d_px], 8, 0, [d_keys], [d_val], 4, outs=[d_out]))
    row(what, "map, 4-byte values", nk, t, 8 * n + 8 * nk, f"table of {8 * slots / 2 ** 20:.0f} MiB")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
