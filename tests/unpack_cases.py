"""The case table of unpack_kernel and pack_kernel (csrc/unpack.hip): named, seeded inputs at the smallest shapes at which each path
of the two kernels can still go wrong, with the format, the reason in one line and the oracle's answer (oracle/pixels.py).  Shared by
the CPU check of the table (tests/test_unpack_cases.py), the emulator (tests/test_emu_unpack.py, tools/emu/emu_unpack.cpp -- which
reads the table from the file `dump` writes and restates nothing of it) and the device (tests/test_gpu_unpack_cases.py).
Importable without a GPU; everything is generated, seeded by a stable function of the case name.

What the shapes are about (the numbers are the kernels': four pixels -- a quad -- per thread, 256 threads per workgroup, a workgroup per
4096 pixels of the largest image of a call, 4096 workgroups at most, a wave of 64 lanes = 256 pixels):
  tails       n % 4 = 1, 2, 3: the last quad is partly filled (`m < 4`), every output layout has its own narrow stores for it
  turns       more than 1024 pixels: a thread comes round again (`q += gridDim.x * blockDim.x`), up to four times; more than
              16 Mi pixels: the cap of 4096 workgroups adds turns
  waves       255 / 256 / 257 quads around the last full wave; 63 / 64 / 65 quads for pack's store of 3- and 6-byte pixels through
              LDS, taken only by a wave all of whose quads are full and whose first storage byte lies on a 16-byte boundary
  offsets     `at`: (bytes of the input, bytes of the output) behind a 16-byte boundary: 1 - 3 turn off the 16-byte and dword
              paths chosen by `& 3`, 4 / 8 / 12 only the store through LDS
"""
from __future__ import annotations

import struct
import sys
import zlib
from dataclasses import dataclass

import numpy as np

import pnghelp as ph

sys.path.insert(0, str(ph.ROOT / "oracle"))
import pixels as orc  # noqa: E402

RGBA, VA, SCALAR = orc.RGBA, orc.VA, orc.SCALAR
LAYOUTS = (RGBA, VA, SCALAR)
P, P8, S, S8 = orc.PREMULTIPLY, orc.PREMULTIPLY_AS_U8, orc.STRAIGHTEN, orc.STRAIGHTEN_AS_U8
BEYOND = (0, 0, 0, 0)                # what the device reads at an index the palette does not hold (the reference traps: oracle/pixels.py)

FORMATS = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (8, 2), (16, 2), (8, 3), (16, 3), (8, 4), (16, 4)]
TAILS = [(1, 1), (3, 1), (5, 3), (257, 31)]                    # n % 4 = 1, 3, 3, 3 ... and (2, 1), (6, 1) below: 2
TURNS = [(1023, 17)]                                            # 5 workgroups whose threads come round three or four times
WAVES = [(255 * 4, 1), (256 * 4, 1), (257 * 4, 1)]              # quads either side of the last full wave of a workgroup
SIZES = TAILS + [(2, 1), (6, 1)] + TURNS + WAVES
# pack's store through LDS (3- and 6-byte pixels): 63, 64 and 65 quads, and a quad short of / a pixel beyond a full wave
STAGED = [(63 * 4, 1), (64 * 4, 1), (65 * 4, 1), (64 * 4 - 1, 1), (64 * 4 + 1, 1), (4 * 64 * 4 - 3, 1)]
PACK_SIZES = SIZES + STAGED
HUGE = (4097, 4096)                                             # above 4096 workgroups x 4096 pixels: the only large case
OFFSETS = (0, 1, 2, 3, 4, 8, 12)
OFFSET_SIZE = (131, 5)                                          # 655 pixels = 163 quads and three pixels: two full waves, a partly filled one


# (file, line that must still be there): the table fails, instead of silently losing coverage, when one of the lines its shapes
# are built around moves
SOURCE_LINES = [
    ("unpack.hip", "const uint64_t quads = (n + 3) / 4;"),
    ("unpack.hip", "const uint32_t m = n - i0 < 4 ? (uint32_t)(n - i0) : 4u;"),
    ("unpack.hip", "for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {"),
    ("unpack.hip", "((uintptr_t)job.storage & 3) == 0;"),
    ("unpack.hip", "(((uintptr_t)job.storage | (uintptr_t)job.pixels) & 3) == 0;"),
    ("unpack.hip", "const bool words = ((uintptr_t)job.storage & 3) == 0;"),
    ("unpack.hip", "((uintptr_t)job.pixels & 3) == 0;"),
    ("unpack.hip", "if ((per == 3 || per == 6) && (q0 + 64) * 4 <= n && ((uintptr_t)(job.storage + q0 * 4 * per) & 15) == 0) {"),
    ("unpack.hip", "if (idx < job.palette_count) {"),
    ("host_colour.hip", "HIP_TRY(launch_unpack(a.dev<UnpackJob>(jslot), count, blocks_for(maxpix, 4096), target, c->stream));"),
    ("host_colour.hip", "HIP_TRY(launch_pack(a.dev<PackJob>(jslot), count, blocks_for(maxpix, 4096), source, c->stream));"),
]
PER_BLOCK, BLOCK = 4096, 256         # pixels of the largest image per workgroup (host_colour.hip), threads per workgroup


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                        # "unpack": storage -> pixels;  "pack": pixels -> storage
    width: int
    height: int
    depth: int
    channels: int
    bits: int                        # T: the target of unpack, the source of pack
    layout: int = RGBA
    indexed: bool = False
    bgr: bool = False
    premultiply: int = 0
    key: tuple | None = None
    palette_count: int = -1          # indexed formats: entries of the palette (`palette(case)`)
    content: str = "noise"           # how `source(case)` fills the input
    at: tuple = (0, 0)               # bytes of (input, output) behind a 16-byte boundary
    reason: str = ""

    @property
    def n(self):
        return self.width * self.height

    @property
    def huge(self):
        return (self.width, self.height) == HUGE

    @property
    def storage_bytes(self):
        return self.n * (1 if self.indexed else self.channels * (2 if self.depth == 16 else 1))

    @property
    def pixel_bytes(self):
        return self.n * {RGBA: 4, VA: 2, SCALAR: 1}[self.layout] * (self.bits // 8)


def _rng(case: Case, salt: str = ""):
    return np.random.default_rng(zlib.crc32((case.name + salt).encode()))


def _pool():
    """512 distinct colours: what the palettes of the pack cases are drawn from, and their strangers -- so that a pixel no entry of
    its own palette equals is an entry of a neighbouring job's"""
    rng = np.random.default_rng(512)
    pool = np.unique(rng.integers(0, 256, (2048, 4), dtype=np.uint8), axis=0)
    return pool[rng.permutation(len(pool))[:512]]


def palette(case: Case) -> bytes | None:
    """palette_count distinct (r, g, b, a) entries (pack cases: of the pool); content "alphas": the alphas run through 0, 1, 254, 255"""
    if not case.indexed:
        return None
    rng = _rng(case, "/palette")
    pal = _pool() if case.kind == "pack" else np.unique(rng.integers(0, 256, (1024, 4), dtype=np.uint8), axis=0)
    pal = pal[rng.permutation(len(pal))[:case.palette_count]]
    assert len(pal) == case.palette_count
    if case.content == "alphas":
        pal[:, 3] = np.array([0, 1, 254, 255], dtype=np.uint8)[np.arange(len(pal)) % 4]
        pal[:, :3] |= 1                                             # (no colour is zero: premultiplied by 0 and by 1 differ)
        assert len(np.unique(pal, axis=0)) == len(pal)
    if case.content == "repeats":
        pal[len(pal) // 2:] = pal[:len(pal) - len(pal) // 2]           # every colour of the upper half stands in the lower half too
    return pal.tobytes()


def storage(case: Case) -> bytes:
    """the input of an unpack case"""
    assert case.kind == "unpack"
    rng, n = _rng(case), case.n
    if case.indexed:
        if case.content == "beyond":
            # indices on both sides of palette_count (a byte holds them whatever the depth says), the two next to it among them
            c = case.palette_count
            idx = rng.integers(0, 256, n)
            if c:
                idx = np.where(rng.random(n) < 0.4, rng.integers(0, c, n), idx)
            near = np.array([v for v in (0, c - 1, c, c + 1, 255) if 0 <= v <= 255])
            idx[:len(near)] = near[:n]
            return idx.astype(np.uint8).tobytes()
        return rng.integers(0, case.palette_count, n).astype(np.uint8).tobytes()
    hi = 1 << case.depth
    atoms = rng.integers(0, hi, (n, case.channels))
    if case.content == "keyed":
        key, colors = np.array(case.key[:case.channels]), case.channels
        kind = rng.integers(0, 10, n)
        atoms[kind == 0] = key                                      # hits
        for z in range(colors):                                     # near misses: one channel off by one, one channel anything else
            sel = kind == 1
            sel &= rng.integers(0, colors, n) == z
            atoms[sel] = key
            atoms[sel, z] = (key[z] + rng.choice([-1, 1], int(sel.sum()))) % hi
        if case.depth == 16:
            sel = kind == 2                                         # equal in the high byte of every channel only
            atoms[sel] = key ^ rng.integers(1, 256, (int(sel.sum()), colors))
            sel = kind == 3                                         # equal in the low byte only
            atoms[sel] = key ^ (rng.integers(1, 256, (int(sel.sum()), colors)) << 8)
        if colors == 3:
            atoms[kind == 4] = key[::-1]                            # the key in the other order
        # the first pixels hold one of each, whatever the draw gave
        planted = [key.copy()]
        for z in range(colors):
            miss = key.copy(); miss[z] = (key[z] + 1) % hi
            planted.append(miss)
        if case.depth == 16:
            planted += [key ^ 0x0001, key ^ 0x0100]
        if colors == 3:
            planted.append(key[::-1].copy())
        if n >= len(planted):
            atoms[:len(planted)] = np.array(planted)
    if case.depth == 16:
        return atoms.astype(">u2").tobytes()
    return atoms.astype(np.uint8).tobytes()


def pixels(case: Case) -> np.ndarray:
    """the input of a pack case: (n, 4) | (n, 2) | (n,) of uint8 / uint16"""
    assert case.kind == "pack"
    rng, n = _rng(case), case.n
    dt = np.uint8 if case.bits == 8 else np.uint16
    k = {RGBA: 4, VA: 2, SCALAR: 1}[case.layout]
    if case.indexed:
        # four in five pixels are entries of the palette as this layout sees them, the others strangers (index 0): colours of the pool,
        # which the palettes of the other cases hold
        pal = np.frombuffer(palette(case), dtype=np.uint8).reshape(-1, 4).astype(np.uint32)
        px = pal[rng.integers(0, len(pal), n)]
        strangers = rng.random(n) < 0.2
        px[strangers] = _pool()[rng.integers(0, 512, int(strangers.sum()))]
        if case.bits == 16:
            px = px << 8 | rng.integers(0, 256, px.shape)           # (the low byte is shifted away)
        px = px[:, {RGBA: [0, 1, 2, 3], VA: [0, 3], SCALAR: [0]}[case.layout]]
    else:
        px = rng.integers(0, 1 << case.bits, (n, k))
    px = px.astype(dt)
    return px[:, 0].copy() if case.layout == SCALAR else px


def source(case: Case) -> bytes:
    """the bytes the kernel reads: storage, or pixels in host (little-endian) order"""
    if case.kind == "unpack":
        return storage(case)
    return pixels(case).astype("<u%d" % (case.bits // 8)).tobytes()


def expected(case: Case) -> bytes:
    """the oracle's answer: pixels in host order, or storage"""
    if case.kind == "unpack":
        out = orc.unpack(storage(case), case.depth, case.channels, indexed=case.indexed, bgr=case.bgr, palette=palette(case),
                         key=None if case.layout == SCALAR else case.key, target=case.bits, layout=case.layout,
                         premultiply=case.premultiply, beyond_palette=BEYOND if case.indexed else None)
        return out.astype("<u%d" % (case.bits // 8)).tobytes()
    px = pixels(case)
    if case.content == "repeats":
        # the reference traps on a palette that holds a colour twice (`pack` refuses it); the device's documented answer is the lowest
        # index: the oracle's for the palette with every later copy replaced by a colour no pixel has (none of the pool)
        pal = np.frombuffer(palette(case), dtype=np.uint8).reshape(-1, 4).copy()
        pool, seen, spare = {tuple(e) for e in _pool()}, set(), (e for e in np.ndindex(256, 256, 256, 256))
        for i, e in enumerate(pal):
            if tuple(e) in seen:
                pal[i] = next(c for c in spare if c not in pool)
            seen.add(tuple(e))
        return orc.pack(px, case.depth, case.channels, indexed=True, palette=pal.tobytes(), layout=case.layout)
    if case.premultiply:
        px = orc.alpha(px, case.bits, case.premultiply)[0].astype(px.dtype)
    return orc.pack(px, case.depth, case.channels, indexed=case.indexed, bgr=case.bgr, palette=palette(case), layout=case.layout)


# ---- the table ----------------------------------------------------------------------------------------------------------------
def _fmt(depth, channels, indexed=False, bgr=False):
    if indexed:
        return "indexed%d" % depth
    return {1: "v", 2: "va", 3: "bgr" if bgr else "rgb", 4: "bgra" if bgr else "rgba"}[channels] + str(depth)


def _formats():
    """the 11 formats, indexed at depths 1, 2, 4, 8, and bgr / bgra: (depth, channels, indexed, bgr)"""
    for depth, channels in FORMATS:
        yield depth, channels, False, False
        if depth == 8 and channels >= 3:
            yield depth, channels, False, True
    for depth in (1, 2, 4, 8):
        yield depth, 1, True, False


def _lname(layout):
    return ("rgba", "va", "scalar")[layout]


def _size_reason(w, h):
    n = w * h
    if (w, h) in TURNS:
        return "several workgroups whose threads come round up to four times; a tail of %d" % (n % 4)
    if (w, h) in WAVES:
        return "%d quads: around the last full wave of a workgroup" % (n // 4)
    if (w, h) in STAGED:
        return "%d quads and %d pixels: the switch between the store through LDS and the plain one" % (n // 4, n % 4)
    return "a tail of %d behind %d full quads" % (n % 4, n // 4)


def _build():
    cases = []
    add = cases.append
    # sizes: every format x both T x the three layouts
    for depth, channels, indexed, bgr in _formats():
        for bits in (8, 16):
            for layout in LAYOUTS:
                for (w, h) in SIZES:
                    add(Case(f"unpack/{_fmt(depth, channels, indexed, bgr)}/u{bits}/{_lname(layout)}/{w}x{h}", "unpack", w, h, depth,
                             channels, bits, layout, indexed, bgr, palette_count=min(1 << depth, 256) if indexed else -1,
                             reason=_size_reason(w, h)))
                if indexed:
                    continue                                        # (pack into indexed formats: below, with their strangers)
                for (w, h) in PACK_SIZES:
                    add(Case(f"pack/{_fmt(depth, channels, indexed, bgr)}/u{bits}/{_lname(layout)}/{w}x{h}", "pack", w, h, depth,
                             channels, bits, layout, indexed, bgr, reason=_size_reason(w, h)))
    # above the cap of 4096 workgroups
    add(Case("unpack/v8/u8/scalar/huge", "unpack", *HUGE, 8, 1, 8, SCALAR, reason="more than 4096 x 4096 pixels: the grid is capped, threads come round a fifth time"))
    add(Case("pack/v8/u8/scalar/huge", "pack", *HUGE, 8, 1, 8, SCALAR, reason="more than 4096 x 4096 pixels: the grid is capped, threads come round a fifth time"))
    # keys
    for depth, channels, bgr, key in ((1, 1, False, (1,)), (2, 1, False, (2,)), (4, 1, False, (9,)), (8, 1, False, (0x80,)),
                                     (16, 1, False, (0x1234,)), (8, 3, False, (0x10, 0x20, 0x30)), (16, 3, False, (0x1234, 0x5678, 0x9abc)),
                                     (8, 3, True, (0x10, 0x20, 0x30))):
        for bits in (8, 16):
            for layout in LAYOUTS:
                add(Case(f"unpack/{_fmt(depth, channels, False, bgr)}/u{bits}/{_lname(layout)}/keyed", "unpack", 61, 7, depth, channels, bits,
                         layout, bgr=bgr, key=key, content="keyed",
                         reason="a tenth of the pixels equal the key, a tenth miss it by one channel" +
                                (", a tenth by one byte of every channel" if depth == 16 else "") +
                                ("; the key as (r, g, b) is no hit, only as it lies in storage" if bgr else "") +
                                ("; the scalar target ignores the key" if layout == SCALAR else "")))
    # indexed: palettes of 0, 1, 2^depth and 256 entries, indices on both sides
    for depth in (1, 2, 4, 8):
        for count in sorted({0, 1, 1 << depth, 256}):
            for bits in (8, 16):
                for layout in LAYOUTS:
                    add(Case(f"unpack/indexed{depth}/u{bits}/{_lname(layout)}/palette{count}", "unpack", 67, 5, depth, 1, bits, layout, True,
                             palette_count=count, content="beyond",
                             reason="indices on both sides of a palette of %d: (0, 0, 0, 0) beyond it" % count))
    # indexed: palette alphas 0, 1, 254, 255 under each operation
    for bits in (8, 16):
        for op in (P, S) + ((P8, S8) if bits == 16 else ()):
            for layout in (RGBA, VA):
                add(Case(f"unpack/indexed8/u{bits}/{_lname(layout)}/alphas/op{op}", "unpack", 67, 5, 8, 1, bits, layout, True, premultiply=op,
                         palette_count=256, content="alphas", reason="palette alphas 0, 1, 254 and 255 under operation %d" % op))
    # the operations on the other formats with alpha, tails included
    for depth, channels, bgr in ((8, 2, False), (16, 2, False), (8, 4, False), (16, 4, False), (8, 4, True)):
        for bits in (8, 16):
            for op in (P, S) + ((P8, S8) if bits == 16 else ()):
                for layout in (RGBA, VA):
                    add(Case(f"unpack/{_fmt(depth, channels, False, bgr)}/u{bits}/{_lname(layout)}/op{op}", "unpack", 131, 5, depth, channels,
                             bits, layout, bgr=bgr, premultiply=op, reason="operation %d fused into the unpack, a tail of 3" % op))
    for depth, channels, bgr in ((8, 4, False), (8, 3, True), (16, 4, False), (8, 2, False)):
        for bits in (8, 16):
            for op in (P,) + ((P8,) if bits == 16 else ()):
                for layout in (RGBA, VA):
                    add(Case(f"pack/{_fmt(depth, channels, False, bgr)}/u{bits}/{_lname(layout)}/op{op}", "pack", 131, 5, depth, channels,
                             bits, layout, bgr=bgr, premultiply=op,
                             reason="operation %d fused into the pack: the 16-byte paths are not taken" % op))
    # pack into indexed formats: different palettes in neighbouring jobs, strangers
    for depth in (1, 2, 4, 8):
        for bits in (8, 16):
            for layout in LAYOUTS:
                add(Case(f"pack/indexed{depth}/u{bits}/{_lname(layout)}/strangers", "pack", 331, 5, depth, 1, bits, layout, True,
                         palette_count=min(1 << depth, 256), reason="a palette of its own; a fifth of the pixels are entries of the other cases' palettes: strangers here, index 0"))
    for depth in (2, 8):
        for bits in (8, 16):
            add(Case(f"pack/indexed{depth}/u{bits}/rgba/repeats", "pack", 331, 5, depth, 1, bits, RGBA, True, palette_count=1 << depth,
                     content="repeats", reason="the upper half of the palette repeats the lower: the lowest index of a colour wins (the reference traps)"))
    # offsets
    for depth, channels, bgr in ((8, 4, False), (8, 4, True), (8, 3, False), (8, 3, True), (16, 3, False), (8, 1, False), (16, 4, False),
                                 (8, 2, False)):
        for bits in (8, 16):
            for layout in LAYOUTS:
                for kind in ("unpack", "pack"):
                    for at in [(o, 0) for o in OFFSETS[1:]] + [(0, o) for o in OFFSETS[1:]]:
                        # pixels of T lie on multiples of T: what spng_pack_batch asks of d_pixels, spng_unpack_batch of d_out
                        if (at[0] if kind == "pack" else at[1]) % (bits // 8):
                            continue
                        add(Case(f"{kind}/{_fmt(depth, channels, False, bgr)}/u{bits}/{_lname(layout)}/at{at[0]}+{at[1]}", kind, *OFFSET_SIZE,
                                 depth, channels, bits, layout, bgr=bgr, at=at,
                                 reason="input %d, output %d bytes behind a 16-byte boundary" % at))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the table as a file: what tools/emu/emu_unpack.cpp reads --------------------------------------------------------------------
def dump(path, want_path, cases):
    """the table and, beside it, the oracle's bytes.  Little-endian.
    table: "UPK1", count; per case: name length, name, 17 x u32 (kind 0 unpack / 1 pack, width, height, depth, channels, bits,
    layout, indexed, bgr, premultiply, has_key, key[3], palette_count, input offset, output offset), u64 input length, u64 output length,
    the palette, the input.  want: per case u64 length and the bytes."""
    with open(path, "wb") as f, open(want_path, "wb") as g:
        f.write(b"UPK1" + struct.pack("<I", len(cases)))
        for c in cases:
            name, src, want, pal = c.name.encode(), source(c), expected(c), palette(c) or b""
            key = (list(c.key or ()) + [0, 0, 0])[:3]
            f.write(struct.pack("<I", len(name)) + name)
            f.write(struct.pack("<17I", c.kind == "pack", c.width, c.height, c.depth, c.channels, c.bits, c.layout, c.indexed, c.bgr,
                                c.premultiply, c.key is not None, *key, len(pal) // 4, *c.at))
            f.write(struct.pack("<QQ", len(src), len(want)) + pal + src)
            g.write(struct.pack("<Q", len(want)) + want)


def groups(cases=None):
    """the cases by the first two parts of their names (kind / format): what tests/golden/unpack_cases.json holds a digest for"""
    g = {}
    for c in CASES if cases is None else cases:
        g.setdefault("/".join(c.name.split("/")[:2]), []).append(c)
    return g


def digest(cases) -> str:
    """of the names, palettes, inputs and oracle's answers of `cases`"""
    import hashlib
    h = hashlib.sha256()
    for c in cases:
        for part in (c.name.encode(), palette(c) or b"", source(c), expected(c)):
            h.update(hashlib.sha256(part).digest())
    return h.hexdigest()
