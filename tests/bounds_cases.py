"""Output capacities that bite: the tables shared by the CPU check of the tables (tests/test_bounds_cases.py), the emulators
(tests/test_emu_bounds.py) and the device tests with guard bytes (tests/test_gpu_bounds.py).  Importable without a GPU; nothing is
read from disk.  What a row must answer is asked of the oracle (pnghelp.orc_inflate / orc_deflate, oracle/gzip_wrap.py), never computed
here; WHERE a capacity lies -- inside a match, on a match's last byte, at a block boundary, inside a stored block, inside a literal
run; inside a header or a trailer, on the staging ring's drain threshold -- is read from the stream's tokens (tests/deflate_tokens.py)
and proven in tests/test_bounds_cases.py.

Inflate: a row is (stream, name of the capacity, capacity).  Deflate: a row is (input, level, format, exponent, name, capacity);
with L the length of the oracle's stream, a capacity below L must answer SPNG_E_OUTPUT_CAPACITY, written == L, consumed == n and the
first `capacity` bytes of the stream (include/spng_mi355.h, spng_deflate_batch)."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

import deflate_cases as dc
import deflate_tokens as dt
import pnghelp as ph
from test_oracle_gzip import gw, raw_deflate, raw_inflate

ZLIB, RAW, GZIP = 0, 1, 2              # spng.FORMAT_ZLIB, FORMAT_IOS, FORMAT_GZIP
E_OUTPUT_CAPACITY = 64
OUTB = 2048                            # csrc/deflate.hip: bytes of the bit writer's staging ring; it drains at OUTB / 2


def scanlines(seed, n):
    """the generator of tests/test_emu_pinflate.py: filtered-scanline-like bytes, every 13th row of 512 noise"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, n).astype(np.int16)
    a[rng.random(n) < 0.6] = 0
    rows = a.astype(np.uint8).reshape(-1, 512)
    rows[::13] = rng.integers(0, 256, (len(rows[::13]), 512), dtype=np.uint8)
    rows[::4, 0] = 1
    return rows.tobytes()


# ---- inflate -----------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Stream:
    name: str
    z: bytes
    fmt: int
    data: bytes
    body_at: int                       # where the raw DEFLATE begins inside z
    body_len: int

    @property
    def n(self):
        return len(self.data)


def _level6(data, wbits):
    """zlib level 6 with 4096 symbols to a block (memLevel 6), so that the 48 KiB make several dynamic blocks"""
    c = zlib.compressobj(6, zlib.DEFLATED, wbits, 6)
    return c.compress(data) + c.flush()


def _raw(data):
    return _level6(data, -15)


def _flushed(data):
    c = zlib.compressobj(6)
    z = b""
    for k, i in enumerate(range(0, len(data), 9000)):
        z += c.compress(data[i:i + 9000]) + c.flush(zlib.Z_FULL_FLUSH if k % 2 == 0 else zlib.Z_SYNC_FLUSH)
    return z + c.flush()


def _gzip_member(data):
    """FEXTRA + FNAME in front of the raw DEFLATE of (a)"""
    raw = _raw(data)
    head = bytes([0x1f, 0x8b, 8, 0x0c, 0, 0, 0, 0, 0, 3]) + (7).to_bytes(2, "little") + b"bounds!" + b"rows.bin\0"
    return head + raw + (zlib.crc32(data) & 0xffffffff).to_bytes(4, "little") + (len(data) & 0xffffffff).to_bytes(4, "little"), len(head), len(raw)


@functools.lru_cache(maxsize=None)
def stream(name) -> Stream:
    a = scanlines(1, 96 * 512)
    if name == "a":
        z = _level6(a, 15)
        return Stream(name, z, ZLIB, a, 2, len(z) - 6)
    if name == "b":
        z = _flushed(a)
        return Stream(name, z, ZLIB, a, 2, len(z) - 6)
    if name == "c":
        noise = np.random.default_rng(31).integers(0, 256, 30000, dtype=np.uint8).tobytes()
        z = zlib.compress(noise, 0)
        return Stream(name, z, ZLIB, noise, 2, len(z) - 6)
    if name in ("periods", "echo"):
        c = dc.case(name)
        return Stream(name, c.stream, ZLIB, c.info["data"], 2, len(c.stream) - 6)
    if name == "a-raw":
        z = _raw(a)
        return Stream(name, z, RAW, a, 0, len(z))
    if name == "a-gzip":
        z, at, n = _gzip_member(a)
        return Stream(name, z, GZIP, a, at, n)
    raise KeyError(name)


STREAMS = ["a", "b", "c", "periods", "echo", "a-raw", "a-gzip"]


@functools.lru_cache(maxsize=None)
def blocks(name):
    st = stream(name)
    return dt.read(st.z[st.body_at:st.body_at + st.body_len], raw=True)


def _first(cands, used):
    for c in cands:
        if c not in used:
            return c
    return None


@functools.lru_cache(maxsize=None)
def inflate_rows(name):
    """-> [(capacity name, capacity)] of a stream, no capacity twice.  The named positions come from the tokens; a name a stream has
    no place for (a match in stored blocks, a stored byte in coded ones, 32768 in 30 000 bytes) is left out."""
    st, blks = stream(name), blocks(name)
    N = st.n
    rows = [("N", N), ("N+1", N + 1), ("N-1", N - 1), ("N-15", N - 15), ("N-16", N - 16), ("N-17", N - 17),
            ("0", 0), ("1", 1), ("15", 15), ("16", 16), ("17", 17)]
    if N > 32769:
        rows += [("32768", 32768), ("32769", 32769)]
    used = {c for _, c in rows}

    def add(label, cands):
        c = _first(cands, used)
        if c is not None:
            used.add(c)
            rows.append((label, c))

    ms = dt.matches(blks)
    if name == "periods":
        add("inside-match", [dc.case("periods-capacity").cap])                   # (the row tests/deflate_cases.py already has)
    elif ms:
        longest = max(m[1] for m in ms)
        add("inside-match", [m[0] + m[1] // 2 for m in ms if m[1] == longest and m[0] > N // 3])
    add("match-end", [m[0] + m[1] for m in ms if N // 2 < m[0] + m[1] < N])
    add("block-boundary", [b.terms[0][0] for b in blks[1:] if b.terms and 0 < b.terms[0][0] < N])
    stored = [b for b in blks if b.kind == "stored"]
    add("inside-stored", [b.terms[0][0] + b.count // 2 for b in stored if b.count >= 3])
    add("at-empty-stored", [_position(blks, k) for k, b in enumerate(blks) if b.kind == "stored" and not b.count and 0 < _position(blks, k) < N])
    lit = []
    for b in blks:
        if b.kind == "stored":
            continue
        t = b.terms
        lit += [t[i][0] for i in range(1, len(t) - 1) if len(t[i - 1]) == 2 and len(t[i]) == 2 and len(t[i + 1]) == 2 and t[i][0] > 64]
        if len(lit) > 4096:
            break
    add("inside-literals", [p for p in lit if p > N // 4] + lit[len(lit) // 2:])        # (deep in the stream where it has literals there)
    return rows


def _position(blks, k):
    """output position at which block k begins"""
    for b in reversed(blks[:k]):
        if b.terms:
            t = b.terms[-1]
            return t[0] + (t[1] if len(t) == 3 else 1)
    return 0


def inflate_expected(name, cap):
    """the oracle's (status, bytes, consumed, aux) of a stream at a capacity"""
    st = stream(name)
    if st.fmt == GZIP:
        return gw.inflate(st.z, lambda p, _c: raw_inflate(p, cap), cap)
    return ph.orc_inflate(st.z, st.fmt, cap=cap)


# ---- deflate -----------------------------------------------------------------------------------------------------------------------

LEVELS = [0, 1, 4, 6, 7, 8, 9, 13]
FAMILY_LEVELS = [1, 6, 9]              # one per family: greedy (0-3), lazy (4-7), full search (8 and up)


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(41)
    text = (b"A wrong bound is silent memory corruption in the caller's neighbouring buffer; a bit-exact comparison of what was "
            b"written cannot see it. " * 2)[:200]
    noise = rng.integers(0, 256, 2500, dtype=np.uint8).tobytes()
    d = {"n%d" % n: bytes(range(65, 65 + n)) for n in range(5)}
    d["text200"] = text
    d["mix5000"] = noise + (text[:50] * 50)[:2500]
    d["scan70000"] = scanlines(2, 137 * 512)[:70000]
    d["noise40000"] = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    assert [len(v) for v in d.values()] == [0, 1, 2, 3, 4, 200, 5000, 70000, 40000]
    return d


INPUTS = ["n0", "n1", "n2", "n3", "n4", "text200", "mix5000", "scan70000", "noise40000"]
SMALL_INPUTS = INPUTS[:7]              # up to 5000 bytes: what the emulator runs at every level


@functools.lru_cache(maxsize=None)
def full(name, level, fmt, exponent=15):
    """the oracle's whole stream"""
    data = inputs()[name]
    if fmt == GZIP:
        return gw.deflate(data, raw_deflate(level))
    return ph.orc_deflate(data, level, fmt, exponent)


SOMETIMES = ("1023", "1024", "1025", "2049")       # kept where L allows: a capacity below L


def deflate_caps(L):
    """-> ([(capacity name, capacity)], names dropped because L is too short for them)"""
    rows = [("L", L), ("L+1", L + 1), ("L-1", L - 1), ("L-4", L - 4), ("L-5", L - 5), ("L-8", L - 8), ("L-9", L - 9), ("0", 0), ("1", 1), ("2", 2),
            ("9", 9), ("10", 10), ("1023", 1023), ("1024", 1024), ("1025", 1025), ("2049", 2049), ("L//2|1", L // 2 | 1)]
    kept, dropped = [], []
    for label, c in rows:
        if c < 0 or (label in SOMETIMES and c >= L):
            dropped.append(label)
        else:
            kept.append((label, c))
    return kept, dropped


def deflate_streams(level):
    """-> [(input, level, format, exponent)] of a level: every input as zlib, raw and gzip at exponent 15, and the 70 000-byte input at
    exponent 8 once per level family"""
    out = [(name, level, fmt, 15) for name in INPUTS for fmt in (ZLIB, RAW, GZIP)]
    if level in FAMILY_LEVELS:
        out.append(("scan70000", level, ZLIB, 8))
    return out


def deflate_rows(level, names=None):
    """-> [(input, level, format, exponent, capacity name, capacity)]"""
    out = []
    for name, lv, fmt, e in deflate_streams(level):
        if names is not None and name not in names:
            continue
        for label, c in deflate_caps(len(full(name, lv, fmt, e)))[0]:
            out.append((name, lv, fmt, e, label, c))
    return out


def deflate_expected(name, level, fmt, exponent, cap):
    """-> (status, written, consumed, the bytes the destination must begin with)"""
    f = full(name, level, fmt, exponent)
    n = len(inputs()[name])
    return (0 if cap >= len(f) else E_OUTPUT_CAPACITY), len(f), n, f[:min(cap, len(f))]
