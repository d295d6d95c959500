"""numpy restatement of what spng_census_batch and spng_pack_indexed_batch compute: the key of a pixel (its components after the
optional premultiplication, PNG.premultiply, Sources/PNG/PNG.swift:55-66, reduced to UInt8 as PNG.deconvolve does, :829-852), the
distinct keys with their frequencies, and the pack through a key -> index map.  Pixels are (n, 4) RGBA, (n, 2) VA or (n,) scalar
arrays of uint8 / uint16."""
import numpy as np

RGBA, VA, SCALAR = 0, 1, 2
PREMULTIPLY, PREMULTIPLY_AS_U8 = 1, 2


def _columns(px, layout):
    px = np.asarray(px)
    return px.reshape(-1, (4, 2, 1)[layout]).astype(np.uint64)


def premultiplied(px, bits, layout, mode):
    """pixels.map(\\.premultiplied) (mode 1) / .premultiplied(as: UInt8.self) (mode 2, bits 16), same shape and type"""
    c = _columns(px, layout)
    if mode == PREMULTIPLY:
        m = (1 << bits) - 1
        c[:, :-1] = (c[:, :-1] * c[:, -1:] + (m >> 1)) // m
    elif mode == PREMULTIPLY_AS_U8:
        c >>= 8
        c[:, :-1] = (c[:, :-1] * c[:, -1:] + 127) // 255
        c *= 257
    return c.astype(np.asarray(px).dtype).reshape(np.asarray(px).shape)


def keys(px, bits, layout, premultiply=0):
    """the uint32 key of every pixel: r | g << 8 | b << 16 | a << 24, v | a << 8, or v, of the UInt8 aggregate"""
    if premultiply:
        px = premultiplied(px, bits, layout, premultiply)
    c = _columns(px, layout) >> (bits - 8)
    k = np.zeros(len(c), dtype=np.uint64)
    for z in range(c.shape[1]):
        k |= c[:, z] << (8 * z)
    return k.astype(np.uint32)


def census(px, bits, layout, premultiply=0):
    """-> (distinct keys ascending, their counts)"""
    k, n = np.unique(keys(px, bits, layout, premultiply), return_counts=True)
    return k.astype(np.uint32), n.astype(np.uint64)


def pack_indexed(px, bits, layout, map_keys, map_indices, miss=0, premultiply=0):
    """-> (one index byte per pixel, pixels whose key is not in the map)"""
    table = {int(k): int(i) for k, i in zip(map_keys, map_indices)}
    k = keys(px, bits, layout, premultiply)
    uniq, inverse = np.unique(k, return_inverse=True)
    hit = np.array([int(u) in table for u in uniq], dtype=bool)
    val = np.array([table.get(int(u), miss) for u in uniq], dtype=np.uint8)
    return val[inverse].astype(np.uint8), int((~hit[inverse]).sum()) if len(k) else 0


def aggregate(key, layout):
    """the tuple (or scalar) the reference hands to an indexer for a key"""
    key = int(key)
    if layout == RGBA:
        return (key & 255, key >> 8 & 255, key >> 16 & 255, key >> 24 & 255)
    if layout == VA:
        return (key & 255, key >> 8 & 255)
    return key & 255
