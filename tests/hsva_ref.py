"""The three conversions of the reference's custom colour target (Snippets/PNG/CustomColor.swift:19-78: struct HSVA { h: UInt32,
s: UInt16, v: UInt8, a: UInt8 }) restated in numpy integers, with plain `//` and `%`: what the device is compared with.

Swift's shifts bind tighter than `/`, `+` and `-`:  .init(mid - min) << 16 / d + 1  is  ((mid - min) << 16) / d + 1.  Not product code."""
import numpy as np

HSVA = np.dtype([("h", "<u4"), ("s", "<u2"), ("v", "u1"), ("a", "u1")])    # the struct in memory: 8 bytes
assert HSVA.itemsize == 8
FROM_RGBA8, TO_RGBA8, TO_VA8 = 1, 2, 3

# sector by (r < g) << 2 | (g < b) << 1 | (r < b), the switch of CustomColor.swift:23-31 row by row:
#   (true, true, _) 3   (false, true, true) 4   (false, true, false) 5   (true, false, true) 2   (true, false, false) 1   (false, false, _) 0
_SECTOR = np.array([0, 0, 5, 4, 1, 2, 3, 3], dtype=np.int64)


def from_rgba(rgba):
    """(n, 4) integers r, g, b, a -> HSVA records (HSVA.init(r:g:b:a:), CustomColor.swift:19-49)"""
    px = np.asarray(rgba).astype(np.int64).reshape(-1, 4)
    r, g, b, a = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    sector = _SECTOR[(r < g).astype(np.int64) << 2 | (g < b).astype(np.int64) << 1 | (r < b).astype(np.int64)]
    lo, hi = np.minimum(np.minimum(r, g), b), np.maximum(np.maximum(r, g), b)
    mid = r + g + b - lo - hi                         # (every case of the switch lists the components in ascending order)
    d = hi - lo
    dd, mm = np.maximum(d, 1), np.maximum(hi, 1)
    f = ((mid - lo) << 16) // dd + 1
    rem = np.where(sector & 1 == 0, f, 65537 - f)
    out = np.zeros(len(px), dtype=HSVA)
    out["h"] = np.where(d > 0, 65537 * sector + rem, 0)
    out["s"] = np.where(d > 0, ((d << 16) - 1) // mm, 0)
    out["v"] = hi
    out["a"] = a
    return out


def to_rgba(hsva):
    """HSVA records -> ((n, 4) uint8 r, g, b, a; boolean mask of the pixels the reference traps on: fatalError("unreachable"),
    sector >= 6 with s > 0 and v > 0 -- they are (v, v, v, a), the device's documented answer) (HSVA.rgba, CustomColor.swift:51-78)"""
    p = np.asarray(hsva, dtype=HSVA).reshape(-1)
    h, s, v, a = (p[k].astype(np.int64) for k in ("h", "s", "v", "a"))
    sector, rem = h // 65537, h % 65537
    f = np.where(sector & 1 == 0, rem, 65537 - rem)
    d = ((s * v) >> 16) + 1
    x, y = v, v - d
    z = ((f * d) >> 16) + y
    grey = (s == 0) | (v == 0)
    trap = ~grey & (sector >= 6)
    perm = {0: (x, z, y), 1: (z, x, y), 2: (y, x, z), 3: (y, z, x), 4: (z, y, x), 5: (x, y, z)}
    out = np.stack([v, v, v, a], axis=1)
    for k, cols in perm.items():
        m = ~grey & (sector == k)
        for c in range(3):
            out[m, c] = cols[c][m]
    assert not out.size or (out.min() >= 0 and out.max() <= 255)                   # (nothing else can trap: d <= v, z <= 255)
    return out.astype(np.uint8), trap


def to_va(hsva):
    """HSVA records -> (n, 2) uint8 v, a: what HSVA.pack stores for the grey formats (CustomColor.swift:232-251)"""
    p = np.asarray(hsva, dtype=HSVA).reshape(-1)
    return np.stack([p["v"], p["a"]], axis=1)


def convert(op, data):
    """bytes or records in, (bytes out, trapped pixels)"""
    if op == FROM_RGBA8:
        return from_rgba(np.frombuffer(bytes(data), dtype=np.uint8).reshape(-1, 4)).tobytes(), 0
    rec = np.frombuffer(bytes(data), dtype=HSVA)
    if op == TO_RGBA8:
        out, trap = to_rgba(rec)
        return out.tobytes(), int(trap.sum())
    return to_va(rec).tobytes(), 0


def tutorial_edits(hsva):
    """the four images the tutorial saves (CustomColor.swift:316-341), by name"""
    p = np.asarray(hsva, dtype=HSVA)
    hue, sat, val = p.copy(), p.copy(), p.copy()
    hue["s"], hue["v"] = 65535 // 2, 255                                           # (h: $0.h, s: .max / 2, v: .max, a: $0.a)
    sat["h"], sat["v"] = 370000, 255                                               # (h: 370000, s: $0.s, v: .max, a: $0.a)
    val["h"], val["s"] = 0, 0                                                      # (h: 0, s: 0, v: $0.v, a: $0.a)
    return {"CustomColor-hue.png": hue, "CustomColor-saturation.png": sat, "CustomColor-value.png": val, "CustomColor.png.png": p}
