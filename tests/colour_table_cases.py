"""The case table of the wide census and the map (csrc/colour_tables.hip: spng_census_wide_batch, spng_map_batch): named, seeded
inputs at the smallest sizes that still reach each rule, each stating what it claims -- the number of distinct keys, and the threshold
it straddles or the rule it plants.  tests/test_colour_table_cases.py holds every case to its claim with numpy (no GPU);
tests/test_gpu_colour_tables.py runs them on the device against tests/indexing_ref.py (census) and a gather through np.searchsorted
(map).  Importable without a GPU; everything is generated, seeded by a stable function of the case name.

The numbers the sizes are built around: census_kernel and map_kernel take four pixels -- a quad -- per lane and 256 lanes per
workgroup (1024 pixels a round); the old finish sorts up to CENSUS_FINISH_LDS_KEYS = 4096 keys in LDS and the wide one
CENSUS_WIDE_TILE = 4096 elements per workgroup, every stride from there on being a launch over the whole buffer; the old entries stop
at 65 536 keys; maps of up to MAP_LDS_KEYS = 512 keys sit in LDS, larger ones in a hash table in scratch."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

import indexing_ref as ref

RGBA, VA, SCALAR = ref.RGBA, ref.VA, ref.SCALAR
MASK = {RGBA: 0xFFFFFFFF, VA: 0xFFFF, SCALAR: 0xFF}
TILE, OLD_CEILING, MAP_LDS_KEYS, WIDE_CAP = 4096, 65536, 512, 1 << 24
MISS = 0xF1E2D3C4B5A69788                                       # a miss value whose bytes all differ (its low value_bytes bytes are used)


def dtype_of(bits):
    return "<u1" if bits == 8 else "<u2"


def pixels_of(keys, bits, layout, rng):
    """pixels of T whose keys (without premultiplication) are `keys`; T = UInt16: random low bytes"""
    keys = np.asarray(keys, dtype=np.uint64)
    c = np.stack([(keys >> np.uint64(8 * z)) & np.uint64(255) for z in range((4, 2, 1)[layout])], axis=1)
    if bits == 16:
        c = c << np.uint64(8) | rng.integers(0, 256, c.shape, dtype=np.uint64)
    return np.ascontiguousarray(c.astype(dtype_of(bits)))


def distinct(n, layout, rng, avoid=()):
    """n distinct keys of the layout, in random order, none of `avoid`"""
    space = MASK[layout] + 1
    if n > space // 4:
        k = rng.permutation(space).astype(np.uint32)
    else:
        k = np.unique(rng.integers(0, space, 2 * n + 64, dtype=np.uint64)).astype(np.uint32)
        k = rng.permutation(k)
    if len(avoid):
        k = k[~np.isin(k, np.asarray(avoid, dtype=np.uint32))]
    assert len(k) >= n
    return k[:n]


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                        # "census" or "map"
    claim: str                       # what the case is there for, in one line
    keys: int                        # census: distinct keys of the pixels;  map: keys of the map (map_count)
    bits: int = 8
    layout: int = RGBA
    premultiply: int = 0
    cap: int = 0                     # census: the cap it is run at (`keys` > cap: SPNG_E_OUTPUT_CAPACITY is the answer)
    offset: int = 0                  # census: bytes of the pixels behind a 16-byte boundary;  map: VALUES of the output behind one
    value_bytes: int = 1             # map
    misses: int = -1                 # map: pixels whose key is not in the map (-1: not claimed)
    duplicate: bool = False          # map: one key is in d_keys twice (device form only); the lowest position wins
    builder: object = field(default=None, compare=False, repr=False)

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.name.encode()))

    def build(self):
        """census: pixels (numpy, one row per pixel).  map: (pixels, map keys ascending uint32, values as uint64 of which the low
        value_bytes bytes count)"""
        return self.builder(self, self.rng())


CASES: list[Case] = []


def add(**kw):
    CASES.append(Case(**kw))


# ---- census ------------------------------------------------------------------------------------------------------------------
def _spread(nk, extra, where="front"):
    """nk distinct keys and `extra` repeats of them: the distinct ones first ("front": whoever reads the first pixels sees them
    all) or last ("back")"""
    def build(c, rng):
        k = distinct(nk, c.layout, rng)
        rep = k[rng.integers(0, nk, extra)] if where != "back" else np.full(extra, k[0], dtype=np.uint32)
        return pixels_of(np.concatenate([k, rep] if where == "front" else [rep, k]), c.bits, c.layout, rng)
    return build


for nk, why in ((1, "one key"), (TILE - 1, "a key below the LDS sort limit"), (TILE, "the LDS sort limit: one tile, no global stride"),
                (TILE + 1, "a key above it: two tiles, the first global stride"), (OLD_CEILING - 1, "a key below the old ceiling"),
                (OLD_CEILING, "the old ceiling itself"), (OLD_CEILING + 1, "the first count the old entry refuses"),
                (131073, "2^17 + 1 keys: 2^18 elements sorted, 21 global strides")):
    add(name=f"census/distinct/{nk}", kind="census", claim=why, keys=nk, cap=max(nk + 7, 16), builder=_spread(nk, 1500))
add(name="census/distinct/2^20+1", kind="census", claim="2^20 + 1 keys in 2^20 + 4099 pixels (4 MiB of RGBA8, the largest case): 2^21 elements, 45 global strides",
    keys=(1 << 20) + 1, cap=(1 << 20) + 4099, builder=_spread((1 << 20) + 1, 4098))
for cap in (OLD_CEILING - 1, OLD_CEILING + 1):
    for extra in (0, 1):
        for where in ("front", "back"):
            add(name=f"census/cap/{cap}/{'over' if extra else 'exact'}/{where}", kind="census", keys=cap + extra, cap=cap,
                claim=("cap + 1 keys: SPNG_E_OUTPUT_CAPACITY, written 0; " if extra else "exactly cap keys fit; ") +
                      ("every key is among the first pixels (the first workgroup's)" if where == "front" else
                       "the pixels of one colour first, every other key among the last (the last workgroup's)"),
                builder=_spread(cap + extra, 3000, where))


def _from_set(make_set, n):
    def build(c, rng):
        s = np.asarray(make_set(c), dtype=np.uint32)
        return pixels_of(np.concatenate([s, s[rng.integers(0, len(s), n)]]), c.bits, c.layout, rng)
    return build


def _random_pixels(n):
    def build(c, rng):
        return rng.integers(0, 1 << c.bits, (n, (4, 2, 1)[c.layout])).astype(dtype_of(c.bits))
    return build


for bits in (8, 16):
    for layout in (RGBA, VA, SCALAR):
        tag = f"u{bits}/{('rgba', 'va', 'v')[layout]}"
        m = MASK[layout]
        add(name=f"census/ends/both/{tag}", kind="census", claim="keys 0x00000000 and all-ones together: neither looks like an empty slot",
            keys=2, cap=2, bits=bits, layout=layout, builder=_from_set(lambda c: [0, MASK[c.layout]], 700))
        add(name=f"census/ends/zero/{tag}", kind="census", claim="key 0 alone", keys=1, cap=1, bits=bits, layout=layout,
            builder=_from_set(lambda c: [0], 300))
        add(name=f"census/ends/ones/{tag}", kind="census", claim="the all-ones key alone (the sort's padding must stay above it)", keys=1, cap=3,
            bits=bits, layout=layout, builder=_from_set(lambda c: [MASK[c.layout]], 300))
        add(name=f"census/bytes/low/{tag}", kind="census", claim="256 keys that differ in the low byte only", keys=256, cap=256, bits=bits,
            layout=layout, builder=_from_set(lambda c: np.arange(256), 1000))
        if layout != SCALAR:
            top = 8 * ((4, 2)[layout] - 1)
            add(name=f"census/bytes/top/{tag}", kind="census", claim="256 keys that differ in the top byte only: the hash must spread them",
                keys=256, cap=300, bits=bits, layout=layout, builder=_from_set(lambda c, top=top: np.arange(256, dtype=np.uint64) << np.uint64(top), 1000))
            for pm in ((1,) if bits == 8 else (1, 2)):
                add(name=f"census/premultiply/{pm}/{tag}", kind="census", claim="the keys of pixels.map(\\.premultiplied): 3001 random pixels",
                    keys=-1, cap=3001, bits=bits, layout=layout, premultiply=pm, builder=_random_pixels(3001))
        step = bits // 8
        for off in sorted({step, 3 * step, 8, 16 - step}):
            add(name=f"census/offset/{off}/{tag}", kind="census", claim="pixels that start off a 16-byte boundary: no vector loads",
                keys=min(40, m + 1), cap=64, bits=bits, layout=layout, offset=off, builder=_spread(min(40, m + 1), 777))
for off in range(1, 16):
    add(name=f"census/offset/{off}/u8/rgba/every", kind="census", claim="RGBA8 at every offset 1 ... 15 from a 16-byte boundary", keys=100, cap=128,
        offset=off, builder=_spread(100, 1031))
add(name="census/flat/70000", kind="census", claim="70 000 pixels of one colour: a count passes 2^16", keys=1, cap=1,
    builder=_from_set(lambda c: [0x80FF8040], 69999))
add(name="census/duplication", kind="census", claim="200 000 pixels drawn from 70 000 colours: merges, and more keys than the old ceiling", keys=70000,
    cap=200000, builder=_spread(70000, 130000))
add(name="census/empty", kind="census", claim="a count of 0: SPNG_DONE, written 0", keys=0, cap=16, builder=lambda c, rng: np.zeros((0, 4), dtype="<u1"))
add(name="census/cap-far-above", kind="census", claim="cap = 2^24 with 5 pixels: scratch is sized by the count", keys=3, cap=WIDE_CAP,
    builder=lambda c, rng: pixels_of([7, 9, 7, 1 << 31, 9], 8, RGBA, rng))


# ---- map -----------------------------------------------------------------------------------------------------------------------
def values_for(keys, value_bytes):
    """a value per key: a multiplicative hash of it, cut to value_bytes"""
    v = (np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xA5A5A5A5A5A5A5A5)
    return v & np.uint64((1 << (8 * value_bytes)) - 1)


def _map(mc, npix, absent=50, ends=None, runs=False, all_miss=False, duplicate=False):
    """a map of mc keys, pixels drawn from them and from `absent` keys that are not in it"""
    def build(c, rng):
        m = MASK[c.layout]
        end_keys = np.array([0, m], dtype=np.uint32)
        keys = distinct(mc, c.layout, rng, avoid=end_keys)
        others = distinct(absent, c.layout, rng, avoid=np.concatenate([keys, end_keys])) if absent else np.zeros(0, dtype=np.uint32)
        pool = np.concatenate([keys, others])
        if ends == "present":
            keys = np.concatenate([keys[:max(mc - 2, 0)], end_keys])[:mc] if mc >= 2 else keys
            pool = np.concatenate([keys, others])
        elif ends == "absent":
            pool = np.concatenate([pool, end_keys])
        if all_miss:
            pool = others
        drawn = pool[rng.integers(0, len(pool), npix)] if len(pool) else np.zeros(npix, dtype=np.uint32)
        if len(others) and not all_miss:                        # a quarter of the pixels miss, however large the map
            drawn = np.where(rng.random(npix) < 0.25, others[rng.integers(0, len(others), npix)], drawn)
        if ends:
            drawn[5:7] = end_keys                               # (pixels of both colours, whatever was drawn)
        if runs:                                                # runs of equal pixels across a lane's quad and a workgroup's tile
            for start, length in ((3, 5), (1022, 7), (2046, 1030)):
                drawn[start:start + length] = drawn[start]
        keys = np.sort(keys)
        if duplicate:                                           # keys[d] twice: positions d and d + 1 hold it, d is the answer
            d = len(keys) // 2
            keys[d + 1] = keys[d]
            drawn[:64] = keys[d]
        values = values_for(np.arange(len(keys)) + 1, c.value_bytes) if duplicate else values_for(keys, c.value_bytes)
        return pixels_of(drawn, c.bits, c.layout, rng), keys.astype(np.uint32), values
    return build


_vb = 0
for mc, why in ((0, "an empty map: every pixel misses"), (1, "one key"), (MAP_LDS_KEYS - 1, "a key below the LDS threshold"),
                (MAP_LDS_KEYS, "the LDS threshold"), (MAP_LDS_KEYS + 1, "the first map in scratch"), (OLD_CEILING, "the old ceiling"),
                (OLD_CEILING + 1, "the first map the old entry refuses"), (131073, "2^17 + 1 keys: a table of 2^19 slots")):
    for vb in (1, 2, 4, 8) if mc in (MAP_LDS_KEYS, MAP_LDS_KEYS + 1) else ((1, 2, 4, 8)[_vb % 4], (1, 2, 4, 8)[(_vb + 2) % 4]):
        add(name=f"map/count/{mc}/v{vb}", kind="map", claim=why, keys=mc, value_bytes=vb, misses=3001 if mc == 0 else -1, offset=1,
            builder=_map(mc, 3001))
    _vb += 1
for ends in ("present", "absent"):
    for mc in (10, MAP_LDS_KEYS + 10):
        for bits, layout in ((8, RGBA), (16, VA)):
            add(name=f"map/ends/{ends}/{mc}/u{bits}/{('rgba', 'va')[layout]}", kind="map", bits=bits, layout=layout, keys=mc, value_bytes=4,
                claim=f"keys 0 and all-ones {ends} in the map, pixels of both colours: neither looks like an empty slot", builder=_map(mc, 1500, ends=ends))
for mc in (40, MAP_LDS_KEYS + 40):
    for vb in (1, 2, 4, 8):
        add(name=f"map/all-miss/{mc}/v{vb}", kind="map", claim="every pixel misses; the miss value's bytes all differ", keys=mc, value_bytes=vb, misses=2051,
            builder=_map(mc, 2051, all_miss=True))
        for off in (1, 3):
            add(name=f"map/offset/{off}/{mc}/v{vb}", kind="map", claim="an output at an odd multiple of value_bytes from a 16-byte boundary: no wide stores",
                keys=mc, value_bytes=vb, offset=off, builder=_map(mc, 1027))
        add(name=f"map/runs/{mc}/v{vb}", kind="map", claim="runs of equal pixels across a lane's quad (3 ... 7, 1022 ... 1028) and a workgroup's tile (2046 ... 3075)",
            keys=mc, value_bytes=vb, builder=_map(mc, 4100, runs=True))
        add(name=f"map/duplicate/{mc}/v{vb}", kind="map", claim="a key present twice in d_keys: its lowest position wins", keys=mc, value_bytes=vb, duplicate=True,
            builder=_map(mc, 1500, duplicate=True))
for bits, layout, pm in ((8, RGBA, 1), (16, RGBA, 2), (16, VA, 1), (8, SCALAR, 0), (16, SCALAR, 0)):
    def _pm(c, rng):
        px = rng.integers(0, 1 << c.bits, (3001, (4, 2, 1)[c.layout])).astype(dtype_of(c.bits))
        keys = np.unique(ref.keys(px, c.bits, c.layout, c.premultiply))[::2]
        return px, keys.astype(np.uint32), values_for(keys, c.value_bytes)
    add(name=f"map/layouts/u{bits}/{('rgba', 'va', 'v')[layout]}/pm{pm}", kind="map", claim="every second key of random pixels, premultiplied where the layout allows",
        keys=-1, bits=bits, layout=layout, premultiply=pm, value_bytes=2, builder=_pm)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def map_oracle(px, c, keys, values):
    """the map as numpy: a gather through np.searchsorted (side="left": the lowest position of a key present twice) -> (values per
    pixel as uint64, misses)"""
    k = ref.keys(px, c.bits, c.layout, c.premultiply)
    miss = np.uint64(MISS & ((1 << (8 * c.value_bytes)) - 1))
    if not len(keys):
        return np.full(len(k), miss, dtype=np.uint64), len(k)
    at = np.searchsorted(keys, k, side="left")
    hit = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == k)
    return np.where(hit, values[np.minimum(at, len(keys) - 1)], miss).astype(np.uint64), int((~hit).sum())
