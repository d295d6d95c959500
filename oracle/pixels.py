"""oracle/pixels.py -- TEST INFRASTRUCTURE, not product code: numpy restatements of the reference's `pack` (pixels ->
PNG.Image.storage), `unpack` (storage -> pixels) and of premultiplied <-> straight alpha: the checkers of `spng_pack_batch`,
`spng_unpack_batch` and `spng_alpha_batch`.  Only tests/, smoke() and bench legs' checkers may import it.

Follows, function by function:
  PNG.RGBA<T>.pack(_:as:indexer:)      Sources/PNG/ColorTargets/PNG.RGBA.swift:409-478
  PNG.VA<T>.pack(_:as:indexer:)        Sources/PNG/ColorTargets/PNG.VA.swift:334-403
  PNG.Image.pack<T>(_:as:indexer:)     Sources/PNG/PNG.Image.swift:767-834        (scalar pixels)
  the default indexers                 Sources/PNG/ColorTargets/PNG.Color.swift:158-226, PNG.Image.swift:1043-1062
  PNG.deconvolve(_:as:depth:kernel:)   Sources/PNG/PNG.swift:1064-1285, :699-745  (big-endian stores)
  PNG.deconvolve(_:reference:kernel:)  Sources/PNG/PNG.swift:819-1062, :748-793   (one byte per pixel)
  PNG.quantum(source:destination:)     Sources/PNG/PNG.swift:255-261

  PNG.RGBA<T>.unpack(_:of:deindexer:)  Sources/PNG/ColorTargets/PNG.RGBA.swift:259-365
  PNG.VA<T>.unpack(_:of:deindexer:)    Sources/PNG/ColorTargets/PNG.VA.swift:184-290
  PNG.Image.unpack<T>(_:of:as:...)     Sources/PNG/PNG.Image.swift:682-760        (scalar pixels)
  the default deindexers               Sources/PNG/ColorTargets/PNG.Color.swift:163-171, :198-206, PNG.Image.swift:1080-1088
  PNG.convolve(_:of:depth:kernel:)     Sources/PNG/PNG.swift:149-204, :495-524 (big-endian loads, quantum / shift)
  PNG.convolve(_:dereference:kernel:)  Sources/PNG/PNG.swift:206-253, :284-466 (one index byte per pixel, UInt8 atoms)
  PNG.premultiply / PNG.straighten     Sources/PNG/PNG.swift:55-66, :101-117; (as: UInt8.self): PNG.RGBA.swift:146-158, :192-206

`unpack` is pinned (tests/test_oracle_unpack.py) on the reference's `.rgba` digests of all PngSuite fixtures and on the iOS goldens.
`pack` is pinned (tests/test_oracle_pack.py) on the reference's own goldens: every `.rgba` file of Sources/PNGIntegrationTests/RGBA
(RGBA<UInt16> pixels) packed as its PNG's format gives back the storage the pinned decode oracle produces for that PNG, and
pack(unpack(storage)) == storage for T = UInt8 wherever the unpack is injective.
"""
from __future__ import annotations

import numpy as np

RGBA, VA, SCALAR = 0, 1, 2


def _transform(v: np.ndarray, tbits: int, depth: int) -> np.ndarray:
    """T -> A at the format's depth (PNG.swift:1076-1095): equal widths as is, narrower T times the quantum, wider T shifted."""
    v = v.astype(np.uint32)
    if tbits == depth:
        return v
    if tbits < depth:
        quantum = ((1 << depth) - 1) // ((1 << tbits) - 1)             # T.max >> (T.bitWidth - destination) / T.max >> (T.bitWidth - source)
        return (quantum * v) & ((1 << depth) - 1)
    return v >> (tbits - depth)


def pack(pixels: np.ndarray, depth: int, channels: int, indexed: bool = False, bgr: bool = False,
         palette: bytes | None = None, layout: int = RGBA) -> bytes:
    """pixels: (n, 4) r g b a | (n, 2) v a | (n,) v, dtype uint8 / uint16  ->  storage bytes."""
    tbits = pixels.dtype.itemsize * 8
    tmax = (1 << tbits) - 1
    px = pixels.reshape(len(pixels), -1).astype(np.uint32)
    n = len(px)
    if layout == RGBA:
        r, g, b, a = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    elif layout == VA:
        r = g = b = px[:, 0]
        a = px[:, 1]
    else:
        r = g = b = px[:, 0]
        a = np.full(n, tmax, dtype=np.uint32)                          # (v, .max), (v, v, v, .max); indexer: (v, v, v, 255)
    if indexed:
        # components as UInt8 atoms (A == UInt8: T wider -> shift), then the default indexer's dictionary; entry 0 for strangers.
        # Dictionary(uniqueKeysWithValues:) traps on a repeated colour (PNG.Color.swift:182-183): refused here as well.
        pal = np.frombuffer(palette, dtype=np.uint8).reshape(-1, 4)
        lookup = {}
        for i, e in enumerate(pal):
            if tuple(e) in lookup:
                raise ValueError("the reference traps: Dictionary(uniqueKeysWithValues:) on a palette that repeats a colour")
            lookup[tuple(int(x) for x in e)] = i
        s = tbits - 8
        keys = np.stack([r >> s, g >> s, b >> s, a >> s], axis=1)
        out = np.fromiter((lookup.get(tuple(int(x) for x in k), 0) for k in keys), dtype=np.uint8, count=n)
        return out.tobytes()
    if channels == 1:
        comps = [r]
    elif channels == 2:
        comps = [r, a]
    elif channels == 3:
        comps = [b, g, r] if bgr else [r, g, b]
    else:
        comps = [b, g, r, a] if bgr else [r, g, b, a]
    atoms = np.stack([_transform(c, tbits, depth) for c in comps], axis=1)
    if depth == 16:
        return atoms.astype(">u2").tobytes()                           # samples[i] = transform(...).bigEndian
    return atoms.astype(np.uint8).tobytes()                            # depth < 8: one unscaled byte per sample in storage


# ---- premultiplied <-> straight alpha ---------------------------------------------------------------------------------------
PREMULTIPLY, PREMULTIPLY_AS_U8, STRAIGHTEN, STRAIGHTEN_AS_U8 = 1, 2, 3, 4      # spng_unpack_desc.premultiply / spng_alpha_desc.op


def alpha(px, bits: int, op: int):
    """px: (n, k) integers, alpha last -> ((n, k) int64 result, components the reference traps on).
    PNG.premultiply / PNG.straighten (PNG.swift:55-66, :101-117) in integers; the (as: UInt8.self) forms (PNG.RGBA.swift:146-158,
    :192-206) work on the high bytes and scale every component, alpha too, back by 257.  Where the reference traps (a > 0 and the
    quotient exceeds T.max) the device's documented answer is T.max: that is what stands in the result."""
    px = np.asarray(px).astype(np.int64)
    c, a, M, scale = px[:, :-1], px[:, -1:], (1 << bits) - 1, 1
    if op in (PREMULTIPLY_AS_U8, STRAIGHTEN_AS_U8):
        if bits != 16:
            raise ValueError("(as: UInt8.self) is a form of T = UInt16")
        c, a, M, scale = c >> 8, a >> 8, 255, 257
    if op in (PREMULTIPLY, PREMULTIPLY_AS_U8):
        out, trapped = (c * a + (M >> 1)) // M, 0                                   # PNG.swift:55-66
    elif op in (STRAIGHTEN, STRAIGHTEN_AS_U8):
        q = (M * c + (a >> 1)) // np.maximum(a, 1)                                  # PNG.swift:101-117
        trap = (a > 0) & (q > M)
        out, trapped = np.where(a == 0, c, np.where(trap, M, q)), int(trap.sum())
    else:
        raise ValueError("no such operation")
    return np.concatenate([out, a], axis=1) * scale, trapped


# ---- unpack -------------------------------------------------------------------------------------------------------------------
def _widen(v: np.ndarray, depth: int, tbits: int) -> np.ndarray:
    """A -> T (PNG.swift:503-522, :292-311): equal widths as is; a wider T: `quantum &* v`, quantum(source: depth, destination:
    T.bitWidth) = T.max / (2^depth - 1) (PNG.swift:255-261), the product wrapping in T; a narrower T: v >> (depth - T.bitWidth)."""
    if tbits == depth:
        return v
    if tbits > depth:
        return (v * np.uint64(((1 << tbits) - 1) // ((1 << depth) - 1))) & np.uint64((1 << tbits) - 1)
    return v >> np.uint64(depth - tbits)


def unpack(storage, depth: int, channels: int, indexed: bool = False, bgr: bool = False, palette: bytes | None = None,
           key=None, target: int = 16, layout: int = RGBA, premultiply: int = 0, beyond_palette=None) -> np.ndarray:
    """storage bytes -> (n, 4) r g b a | (n, 2) v a | (n,) v of dtype uint8 / uint16 (`target` bits), as PNG.RGBA<T>.unpack,
    PNG.VA<T>.unpack and the scalar PNG.Image.unpack<T> with the default deindexers do, in uint64 throughout.

    key: the chroma key of a v / rgb / bgr format, at the format's depth.  It is compared with the samples AS THEY LIE IN STORAGE:
    the kernels of PNG.convolve get the scaled tuple and the original atoms side by side (PNG.swift:176-189), and `.bgr8` tests
    `k == key` on those atoms and swizzles only the output, `.init(c.2, c.1, c.0, ...)` (PNG.RGBA.swift:318-323, PNG.VA.swift:243-248):
    a bgr8 key is (b, g, r).  That is the FORMAT's key, not a file's tRNS chunk: tRNS holds (r, g, b) (PNG.Transparency.swift:154-162)
    and the reference reverses it when it builds `.bgr8` for a CgBI file (PNG.Format.swift:427-430) -- so in a file the pixel whose
    (r, g, b) equals the tRNS key is the keyed one, and whoever forms `key` from a CgBI file's tRNS reverses it (tests/pnghelp.py
    `format_key`).  The scalar target ignores keys (PNG.Image.swift:699-739).
    An index at or beyond the palette's count: the default deindexers subscript a Swift array, `palette[i]` (PNG.Color.swift:169,
    :204, PNG.Image.swift:1086), which traps.  Raised as ValueError here -- unless `beyond_palette` gives the (r, g, b, a) UInt8 entry
    to read there: (0, 0, 0, 0) is the device's documented departure.
    premultiply: 0 or PREMULTIPLY / PREMULTIPLY_AS_U8 / STRAIGHTEN / STRAIGHTEN_AS_U8 applied to every pixel (`alpha`): what
    unpack(as:).map(\\.premultiplied) ... give.  Not with the scalar layout, which has no alpha."""
    if target not in (8, 16) or layout not in (RGBA, VA, SCALAR):
        raise ValueError("target is 8 or 16, layout RGBA / VA / SCALAR")
    if layout == SCALAR and premultiply:
        raise ValueError("a scalar has no alpha")
    raw = np.frombuffer(bytes(storage), dtype=np.uint8)
    tmax = np.uint64((1 << target) - 1)
    if indexed:
        if channels != 1 or depth > 8 or key is not None:
            raise ValueError("indexed formats: one channel of at most 8 bits, no key")
        pal = np.frombuffer(palette or b"", dtype=np.uint8).reshape(-1, 4).astype(np.uint64)
        idx = raw.astype(np.int64)
        beyond = idx >= len(pal)
        if beyond.any() and beyond_palette is None:
            raise ValueError("the reference traps: palette[i] with i beyond the palette")
        pal = np.concatenate([pal, np.array([beyond_palette or (0, 0, 0, 0)], dtype=np.uint64)])
        entry = pal[np.where(beyond, len(pal) - 1, idx)]
        quad = _widen(entry, 8, target)                                 # atoms are UInt8 whatever the format's depth
        r, g, b, a = quad[:, 0], quad[:, 1], quad[:, 2], quad[:, 3]
    else:
        if depth == 16:
            atoms = np.frombuffer(bytes(storage), dtype=">u2").astype(np.uint64).reshape(-1, channels)   # .init(bigEndian:)
        else:
            atoms = raw.astype(np.uint64).reshape(-1, channels)
        c = _widen(atoms, depth, target)
        n = len(c)
        opaque = np.full(n, tmax, dtype=np.uint64)
        if key is not None and channels not in (1, 3):
            raise ValueError("only v, rgb and bgr formats have a key")
        if channels == 1:
            r = g = b = c[:, 0]
            a = opaque if key is None else np.where(atoms[:, 0] == np.uint64(key[0]), np.uint64(0), tmax)
        elif channels == 2:
            r = g = b = c[:, 0]
            a = c[:, 1]
        else:
            r, g, b = (c[:, 2], c[:, 1], c[:, 0]) if bgr else (c[:, 0], c[:, 1], c[:, 2])
            if channels == 4:
                a = c[:, 3]
            elif key is None:
                a = opaque
            else:
                hit = (atoms[:, :3] == np.array(key[:3], dtype=np.uint64)).all(axis=1)      # the storage tuple, not (r, g, b)
                a = np.where(hit, np.uint64(0), tmax)
    dt = np.uint8 if target == 8 else np.uint16
    if layout == SCALAR:
        return r.astype(dt)                                             # the grey value / the red channel / palette[i].r
    px = np.stack([r, g, b, a] if layout == RGBA else [r, a], axis=1)
    if premultiply:
        px = alpha(px, target, premultiply)[0]
    return px.astype(dt)


# ---- PNG.Context.push(data:overdraw: true): progressive display of an unfinished Adam7 image --------------------------------
ADAM7 = [((0, 0), (3, 3)), ((4, 0), (3, 3)), ((0, 4), (2, 3)), ((2, 0), (2, 2)), ((0, 2), (1, 2)), ((1, 0), (1, 1)),
         ((0, 1), (0, 1))]                                                # PNG.adam7 (base, exponent), PNG.Decoder.swift:6-15


def overdrawn(final: np.ndarray, scanlines: int, fill: int = 0) -> np.ndarray:
    """What PNG.Image.storage holds after the first `scanlines` scanlines of an interlaced image went through
    PNG.Context.push(data:overdraw: true) -- scanline by scanline as the reference does it (PNG.Decoder.swift:59-110 order,
    PNG.Context.swift:92-97 brush, PNG.Image.swift:134-183 overdraw; assign = the finished image's pixel).
    final: (H, W, elem) uint8, the finished storage; pixels nothing has reached yet hold `fill`."""
    H, W, _ = final.shape
    img = np.full_like(final, fill)
    left = scanlines
    for (bx, by), (ex, ey) in ADAM7:
        sx, sy = 1 << ex, 1 << ey
        sub_w, sub_h = (W + sx - bx - 1) >> ex, (H + sy - by - 1) >> ey
        if sub_w <= 0 or sub_h <= 0:
            continue
        for y in range(sub_h):
            if left == 0:
                return img
            left -= 1
            base_x, base_y = bx, by + y * sy
            img[base_y, base_x::sx] = final[base_y, base_x::sx]          # assign(scanline:at:stride:)
            s_x, s_y = (0 if base_x == 0 else 1), (0 if base_y & 7 == 0 else 1)
            brush_x, brush_y = sx >> s_x, sy >> s_y
            if brush_x * brush_y <= 1:
                continue
            for yy in range(base_y, min(base_y + brush_y, H)):
                for x in range(base_x, W, brush_x):
                    for xx in range(x, min(x + brush_x, W)):
                        img[yy, xx] = img[base_y, x]
    return img
