"""Shared by the tests of the tutorials' own streams (tests/golden/tutorials.json, written by tests/golden/make_tutorials.py): the
files the reference's tutorials wrote and committed under Sources/PNG/docs.docc/*/, the level each was written at, the CPU oracle's
encoder as one call, and COMPUTE_LUMINANCE of Snippets/PNG/BasicEncoding.swift:63-71 restated in numpy.  Not product code."""
import ctypes
import hashlib

import numpy as np

import pnghelp as ph

DOCS = ph.REFERENCE / "Sources" / "PNG" / "docs.docc"
COPIES = ph.GOLDEN / "tutorials"

# (directory under docs.docc, file, the level its tutorial encoded at)
FILES = [("BasicEncoding", "BasicEncoding-color-rgb@0.png", 0), ("BasicEncoding", "BasicEncoding-color-rgb@4.png", 4),
         ("BasicEncoding", "BasicEncoding-color-rgb@8.png", 8), ("BasicEncoding", "BasicEncoding-color-rgb.png", 9),
         ("BasicEncoding", "BasicEncoding-color-rgb@13.png", 13), ("BasicEncoding", "BasicEncoding-color-v.png", 9),
         ("BasicEncoding", "BasicEncoding-luminance-v.png", 9), ("BasicEncoding", "BasicEncoding-luminance-rgb.png", 9),
         ("BasicDecoding", "BasicDecoding.v.png", 9), ("BasicDecoding", "BasicDecoding.va.png", 9),
         ("OnlineDecoding", "OnlineDecoding-progressive.png", 9), ("ImagesInMemory", "ImagesInMemory.png.png", 13),
         ("Indexing", "Indexing-indexed.png", 9), ("iPhoneOptimized", "iPhoneOptimized-bgr8.png", 9),
         ("iPhoneOptimized", "iPhoneOptimized-rgb8.png", 9), ("ImageMetadata", "ImageMetadata-newtime.png", 9),
         ("CustomColor", "CustomColor-hue.png", 9)]
COPIED = ["BasicEncoding-color-rgb@13.png", "BasicEncoding-luminance-v.png", "OnlineDecoding-progressive.png", "ImagesInMemory.png.png"]
RASTER = "BasicEncoding-color-rgb@13.png"                       # carries the 638 x 425 raster of BasicEncoding.rgba (alpha 255 throughout)
RGB_LEVELS = {0: "BasicEncoding-color-rgb@0.png", 4: "BasicEncoding-color-rgb@4.png", 8: "BasicEncoding-color-rgb@8.png",
              9: "BasicEncoding-color-rgb.png", 13: "BasicEncoding-color-rgb@13.png"}


_encoded = {}


def sha(data) -> str:
    return hashlib.sha256(bytes(data)).hexdigest()


def orc_encode(storage, w, h, depth, channels, interlaced, fmt, level) -> bytes:
    """PNG.Image.compress at `level` by the CPU oracle: the concatenated IDAT.  Remembered by the storage's digest: the rgb raster at
    level 13 takes the oracle most of a minute, and three tests ask for it."""
    lib = ph.oracle()
    storage = np.ascontiguousarray(storage, dtype=np.uint8)
    key = (sha(storage), w, h, depth, channels, int(interlaced), fmt, level)
    if key in _encoded:
        return _encoded[key]
    cap = lib.orc_deflate_bound(lib.orc_inflated_size(w, h, depth, channels, int(interlaced)))
    dst = np.empty(cap, dtype=np.uint8)
    written = ctypes.c_size_t(0)
    st = lib.orc_encode(ph._ptr(storage), w, h, depth, channels, int(interlaced), fmt, level, ph._ptr(dst), cap, ctypes.byref(written))
    assert st == 0, st
    _encoded[key] = dst[:written.value].tobytes()
    return _encoded[key]


def reencode(data: bytes, level: int):
    """a file decoded by the oracle and encoded again at `level`: -> (its Png, the new IDAT)"""
    png = ph.parse_png(data)
    st, storage, _ = ph.orc_decode(png)
    assert st == 0
    return png, orc_encode(storage, png.width, png.height, png.depth, png.channels, png.interlaced, png.fmt, level)


def format_name(png) -> str:
    kind = {0: "v", 2: "bgr" if png.ios else "rgb", 3: "indexed", 4: "va", 6: "bgra" if png.ios else "rgba"}[png.color]
    return f"{kind}{png.depth}"


def luminance(rgb) -> np.ndarray:
    """COMPUTE_LUMINANCE (BasicEncoding.swift:63-71) over (n, >= 3) uint8: IEEE-754 binary64 in the association
    ((0.299 r) r + (0.587 g) g) + (0.114 b) b (numpy neither reassociates nor contracts), the correctly rounded root, halves away from
    zero (Swift's .rounded(); np.round would take them to even), clamped to 0 ... 255.  -> (n,) uint8"""
    c = np.asarray(rgb)[:, :3].astype(np.float64)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    l = np.sqrt(((0.299 * r) * r + (0.587 * g) * g) + (0.114 * b) * b)
    whole = np.floor(l)
    return np.clip(whole + (l - whole >= 0.5), 0, 255).astype(np.uint8)    # (l - whole is exact; l + 0.5 need not be)
