"""A plain DEFLATE reader (RFC 1951, RFC 1950 wrapper) that keeps the tokens: what a compressor DECIDED, which the inflated
bytes no longer show.  Pure Python, no dependency on the product or the oracle; tests/test_encode_cases.py cross-checks it with
zlib.decompress of the same stream.  It does not rebuild the output (a match only needs the position it starts at), so a stream
of a few thousand tokens over megabytes reads in well under a second; bits are taken from a 64-bit-refilled accumulator, symbols
from one flat table per code.

    blocks = read(stream)                # zlib stream (raw=True: bare DEFLATE)
    blocks[k].kind                       # "stored" | "fixed" | "dynamic"
    blocks[k].final, .count              # BFINAL; number of terms (the end-of-block symbol is not a term)
    blocks[k].first_bit, .last_bit       # the block's first header bit and its last bit (of the end-of-block symbol, or of the
                                         #   last stored byte), counted from the start of `stream`
    blocks[k].terms                      # (position, literal) | (position, run, distance)

Anything malformed raises Malformed."""
from __future__ import annotations

from dataclasses import dataclass, field

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Malformed(ValueError):
    pass


@dataclass
class Block:
    kind: str
    final: bool
    first_bit: int
    last_bit: int = 0
    terms: list = field(default_factory=list)

    @property
    def count(self):
        return len(self.terms)

    @property
    def matches(self):
        return [t for t in self.terms if len(t) == 3]


def _table(lengths, what):
    """code lengths -> (flat table indexed by the next `width` bits LSB-first: symbol << 4 | length, or -1; width)"""
    width = max(lengths) if lengths else 0
    if width == 0:
        return [], 0
    count = [0] * (width + 1)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, width + 1):
        left = (left << 1) - count[l]
        if left < 0:
            raise Malformed(f"{what}: over-subscribed code lengths")
    if left > 0 and not (sum(count) == 1 and count[1] == 1):
        raise Malformed(f"{what}: incomplete code lengths")
    code, nxt = 0, [0] * (width + 2)
    for l in range(1, width + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    tab = [-1] * (1 << width)
    for sym, l in enumerate(lengths):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        r = int(format(c, "0%db" % l)[::-1], 2)              # (codes are packed MSB first: RFC 1951 3.1.1)
        n = 1 << (width - l)
        tab[r::1 << l] = [sym << 4 | l] * n
    return tab, width


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "fixed literal/length"), _table([5] * 32, "fixed distance"))
    return _FIXED


class _Bits:
    __slots__ = ("data", "at", "acc", "n")

    def __init__(self, data, byte):
        self.data, self.at, self.acc, self.n = data, byte, 0, 0

    def need(self, k):
        """at least k bits in the accumulator (k <= 48), or as many as the stream still has"""
        if self.n < k:
            chunk = self.data[self.at:self.at + 8]
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.at += len(chunk)
            self.n += 8 * len(chunk)

    def take(self, k):
        self.need(k)
        if self.n < k:
            raise Malformed("the stream ends inside a block")
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    @property
    def pos(self):
        return 8 * self.at - self.n


def _read_lengths(b):
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise Malformed(f"HLIT {hlit} / HDIST {hdist} out of range")
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = b.take(3)
    tab, width = _table(cl, "code length code")
    if not width:
        raise Malformed("no code length code")
    lens = []
    while len(lens) < hlit + hdist:
        b.need(width + 7)
        e = tab[b.acc & ((1 << width) - 1)]
        if e < 0 or (e & 15) > b.n:
            raise Malformed("unassigned code length code" if e < 0 else "the stream ends inside a block")
        b.acc >>= e & 15
        b.n -= e & 15
        sym = e >> 4
        if sym < 16:
            lens.append(sym)
            continue
        if sym == 16:
            if not lens:
                raise Malformed("repeat without a previous length")
            lens += [lens[-1]] * (3 + b.take(2))
        else:
            lens += [0] * (3 + b.take(3) if sym == 17 else 11 + b.take(7))
    if len(lens) > hlit + hdist:
        raise Malformed("a repeat runs over the end of the code lengths")
    if lens[256] == 0:
        raise Malformed("no end-of-block code")
    return _table(lens[:hlit], "literal/length"), _table(lens[hlit:], "distance")


def read(stream: bytes, raw: bool = False):
    """-> list of Block.  zlib streams: header and the presence of the four trailer bytes are checked (the Adler-32 itself is
    zlib.decompress's business)."""
    start = 0
    if not raw:
        if len(stream) < 2:
            raise Malformed("no zlib header")
        cmf, flg = stream[0], stream[1]
        if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
            raise Malformed("bad zlib header")
        start = 2
    b = _Bits(stream, start)
    pos, blocks = 0, []
    while True:
        first_bit = b.pos
        final, kind = b.take(1), b.take(2)
        if kind == 3:
            raise Malformed("reserved block type")
        blk = Block(("stored", "fixed", "dynamic")[kind], bool(final), first_bit)
        if kind == 0:
            b.take(b.n & 7)
            n, c = b.take(16), b.take(16)
            if n ^ c != 0xffff:
                raise Malformed("stored block: LEN / NLEN")
            for _ in range(n):
                blk.terms.append((pos, b.take(8)))
                pos += 1
        else:
            (lt, lw), (dt, dw) = _fixed() if kind == 1 else _read_lengths(b)
            lmask, dmask, terms = (1 << lw) - 1, (1 << dw) - 1, blk.terms
            while True:
                b.need(48)                                     # a whole token: 15 + 5 + 15 + 13 bits
                acc, n = b.acc, b.n
                e = lt[acc & lmask]
                l = e & 15
                if e < 0 or l > n:
                    raise Malformed("unassigned literal/length code" if e < 0 else "the stream ends inside a block")
                acc >>= l
                n -= l
                sym = e >> 4
                if sym < 256:
                    terms.append((pos, sym))
                    pos += 1
                    b.acc, b.n = acc, n
                    continue
                if sym == 256:
                    b.acc, b.n = acc, n
                    break
                if sym > 285:
                    raise Malformed(f"length symbol {sym}")
                x = LEN_EXTRA[sym - 257]
                run = LEN_BASE[sym - 257] + (acc & ((1 << x) - 1))
                acc >>= x
                n -= x
                if not dw:
                    raise Malformed("a match in a block without distance codes")
                e = dt[acc & dmask]
                l = e & 15
                if e < 0 or l > n:
                    raise Malformed("unassigned distance code" if e < 0 else "the stream ends inside a block")
                acc >>= l
                n -= l
                ds = e >> 4
                if ds > 29:
                    raise Malformed(f"distance symbol {ds}")
                x = DIST_EXTRA[ds]
                dist = DIST_BASE[ds] + (acc & ((1 << x) - 1))
                acc >>= x
                n -= x
                if n < 0:
                    raise Malformed("the stream ends inside a block")
                if dist > pos:
                    raise Malformed(f"distance {dist} at position {pos}")
                terms.append((pos, run, dist))
                pos += run
                b.acc, b.n = acc, n
        blk.last_bit = b.pos - 1
        blocks.append(blk)
        if final:
            break
    if not raw and len(stream) - (b.pos + 7) // 8 != 4:
        raise Malformed("zlib trailer: %d bytes behind the last block" % (len(stream) - (b.pos + 7) // 8))
    if raw and len(stream) != (b.pos + 7) // 8:
        raise Malformed("bytes behind the last block")
    return blocks


def matches(blocks):
    """every (position, run, distance) of the stream, in order"""
    return [t for blk in blocks for t in blk.terms if len(t) == 3]


def length(blocks):
    """bytes the stream inflates to"""
    for blk in reversed(blocks):
        if blk.terms:
            t = blk.terms[-1]
            return t[0] + (t[1] if len(t) == 3 else 1)
    return 0
