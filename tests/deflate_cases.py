"""DEFLATE streams that no compressor writes: the case table shared by the CPU check of the table and of both emulators
(tests/test_deflate_cases.py) and the GPU parity tests (tests/test_gpu_deflate_cases.py), so both speak of one definition.
Importable without a GPU.  Every stream is assembled token by token with the writers of tests/oneblock.py from fixed seeds; nothing
is read from disk, and what a stream inflates to is asked of zlib (valid cases) or of the oracle (malformed ones), never computed here.

A compressor only emits what its match finder finds, so these paths of the parallel inflate pipeline (csrc/pinflate2.hip) run on
hand-built tokens only: the period reduction of pinf2_resolve_kernel's expand step at every (run, distance), the cap on a tile's
back-references, the markers of the parts behind the first at a part's very first byte / one byte in front of it / 32768 bytes in
front of it, token fields at their ends, headers zlib does not write, and a malformed block behind 50 KB of good ones.

A case carries its tokens (`blocks`: one token table per block, rows (literal/length symbol, extra bits, distance symbol or -1, extra
bits)) so that tests/test_deflate_cases.py can prove from them, in plain Python, that the case is what it claims."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import oneblock as ob
import pnghelp as ph

ZLIB, RAW = 0, 1                       # spng.FORMAT_ZLIB, spng.FORMAT_IOS; the oracle's formats
HEAD = 32768                           # literals in front, so that every distance is valid


@dataclass(frozen=True)
class Case:
    name: str
    stream: bytes
    fmt: int
    purpose: str
    valid: bool
    body: bytes = b""                  # valid cases: the raw DEFLATE inside the stream (for other wrappers)
    cap: int = 0                       # malformed cases: the output capacity the expectation below holds for
    expect: tuple | None = None        # malformed cases: the oracle's (status, written, (aux0, aux1)), recorded
    blocks: tuple = ()                 # one token table per block (None: a block that has no tokens to speak of)
    info: dict = field(default_factory=dict, hash=False, compare=False)


def runs_and_distances(tokens):
    """token table -> (is reference, bytes the token stands for, distance) per token"""
    t = np.asarray(tokens, np.int64).reshape(-1, 4)
    ref = t[:, 2] >= 0
    run = np.ones(len(t), np.int64)
    run[ref] = ob.LEN_BASE[t[ref, 0] - 257] + t[ref, 1]
    dist = np.zeros(len(t), np.int64)
    dist[ref] = ob.DIST_BASE[t[ref, 2]] + t[ref, 3]
    return ref, run, dist


def _lits(vals):
    vals = np.asarray(vals, np.int64)
    z = np.zeros(len(vals), np.int64)
    return ob.symbol_tokens(vals, z, z)


def _refs(run, dist):
    run, dist = np.asarray(run, np.int64), np.asarray(dist, np.int64)
    return ob.symbol_tokens(np.full(len(run), -1, np.int64), run, dist)


def _block(tokens, final=False, complete=True):
    llen, dlen = ob.token_lengths(tokens, complete)
    return ob.coded_block(llen, dlen, tokens, final=final)


def _valid(name, purpose, blocks, tables, **info):
    body, _ = ob.concat_bits(blocks)
    data = zlib.decompressobj(-15).decompress(body)
    return Case(name, ob.zlib_wrap(body, data), ZLIB, purpose, True, body=body, blocks=tuple(tables), info=dict(info, data=data))


def _malformed(name, purpose, blocks, tables, cap=1 << 20, **info):
    """the trailer is the Adler-32 of what the ORACLE makes of the body: where the reference sees nothing wrong (see fixed-l286), the
    stream then ends well for it"""
    body, _ = ob.concat_bits(blocks)
    st, out, _, _ = ph.orc_inflate(body, RAW, cap=cap)
    return Case(name, ob.zlib_wrap(body, out), ZLIB, purpose, False, cap=cap, expect=EXPECT.get(name), blocks=tuple(tables), info=info)


# ---- the valid cases -----------------------------------------------------------------------------------------------------------

def periods():
    rng = np.random.default_rng(101)
    pairs = [(r, d) for r in range(3, 259) for d in range(1, r)]                 # 1 <= distance < run <= 258: 33 152 of them
    pairs += [(d, d) for d in range(3, 259)] + [(d - 1, d) for d in range(4, 259)]
    pairs = np.array(pairs, np.int64)[rng.permutation(len(pairs))]
    head = _lits(rng.integers(0, 256, 300))
    t = np.zeros((2 * len(pairs), 4), np.int64)
    t[0::2] = _lits(rng.integers(0, 256, len(pairs)))                            # (the period's content changes from run to run)
    t[1::2] = _refs(pairs[:, 0], pairs[:, 1])
    tokens = np.concatenate([head, t])
    return _valid("periods", "every (run, distance) with distance < run: the period reduction of resolve's expand step (v_rcp_f32)",
                  [_block(tokens, final=True)], [tokens])


def _extreme_fields():
    dists = sorted({int(b) + e for b, x in zip(ob.DIST_BASE, ob.DIST_EXTRA) for e in (0, (1 << int(x)) - 1)})
    lens = []                                                                    # (length symbol, extra)
    for k, x in enumerate(ob.LEN_EXTRA):
        lens += [(257 + k, 0)] + ([(257 + k, (1 << int(x)) - 1)] if x else [])
    return dists, lens                                                           # (284, 31) is run 258 written the long way


def extremes():
    rng = np.random.default_rng(102)
    dists, lens = _extreme_fields()
    rows = []
    for d in dists:
        ds = int(np.searchsorted(ob.DIST_BASE, d, side="right") - 1)
        for sym, extra in lens:
            rows.append((sym, extra, ds, d - int(ob.DIST_BASE[ds])))
    rows = np.array(rows, np.int64)[rng.permutation(len(rows))]
    tokens = np.concatenate([_lits(rng.integers(0, 256, HEAD)), rows])
    return _valid("extremes", "token fields at their ends: first and last distance of every distance code x first and last run of every "
                  "length code; distance 32768 (all fifteen bits of distance - 1); run 258 as symbol 285 and as 284 + 31",
                  [_block(tokens, final=True)], [tokens])


def dense(name, seed, mixed):
    rng = np.random.default_rng(seed)
    n = 24000
    dist = rng.integers(1, 32769, n)
    if mixed:
        run = rng.integers(3, 5, n)
        t = _refs(run, dist)
        lit = rng.random(n) < 0.12                                               # single literals dropped in: the references' first
        t[lit] = _lits(rng.integers(0, 256, int(lit.sum())))                     # halfwords move through a thread's eight
    else:
        t = _refs(np.full(n, 3), dist)
    tokens = np.concatenate([_lits(rng.integers(0, 256, 33000)), t])
    return _valid(name, "more than one reference per 8 output bytes across whole tiles: a tile ended by the reference cap (MAXM)"
                  + (", runs 3 and 4 and single literals mixed" if mixed else ", runs of 3 back to back"),
                  [_block(tokens, final=True)], [tokens], head=33000)


def dense_blocks():
    """the same density in 16 blocks: a stream of ONE block is never cut into parts, and only the parts behind the first can run the
    4 KiB geometry, whose cap is 512"""
    rng = np.random.default_rng(107)
    tables = [_lits(rng.integers(0, 256, 33000))]
    for _ in range(16):
        n = 1500
        t = _refs(rng.integers(3, 5, n), rng.integers(1, 32769, n))
        lit = rng.random(n) < 0.12
        t[lit] = _lits(rng.integers(0, 256, int(lit.sum())))
        tables.append(t)
    blocks = [_block(t, final=i == 16) for i, t in enumerate(tables)]
    return _valid("dense-blocks", "the density of dense34 in 16 blocks, so that parts behind the first meet it: the reference cap of the "
                  "4 KiB tiles (512) under markers", blocks, tables, head=33000)


ECHO_BLOCKS = 26


def echo():
    rng = np.random.default_rng(104)
    first = _lits(rng.integers(0, 256, HEAD))
    rep = _refs([258] * 126 + [130, 130], [32768] * 128)                         # 126 x 258 + 130 + 130 = 32768 bytes
    tables = [first] + [rep] * ECHO_BLOCKS
    blocks = [_block(first)] + [_block(rep, final=k == ECHO_BLOCKS - 1) for k in range(ECHO_BLOCKS)]
    bits = np.cumsum([0] + [b[1] for b in blocks])
    return _valid("echo", "128 references at distance 32768 per block: the output is the first 32 KiB over and over; with parts, the last "
                  "part's bytes are markers of markers back to the first part (window and fixup kernels)", blocks, tables,
                  block_bits=[int(b) for b in bits])


EDGE_BLOCKS = 44


def edges():
    rng = np.random.default_rng(105)
    tables = [_lits(rng.integers(0, 256, HEAD))]
    for _ in range(EDGE_BLOCKS):
        r1, r2, r3 = (int(v) for v in rng.integers(3, 259, 3))
        k = int(rng.integers(2, 100))                                            # the fourth source begins k bytes in front of P
        r4 = k + int(rng.integers(1, 258 - k + 1))                               # ... and its run straddles P
        at = r1 + r2 + r3                                                        # (bytes of the block in front of the fourth)
        refs = _refs([r1, r2, r3, r4], [32768, r1 + 1, r1 + r2, at + k])         # sources: P - 32768, P - 1, P, P - k
        tables.append(np.concatenate([refs, _lits(rng.integers(0, 256, int(rng.integers(2600, 3000))))]))
    blocks = [_block(t, final=i == EDGE_BLOCKS) for i, t in enumerate(tables)]
    return _valid("edges", "every block begins with references to P - 32768, P - 1, P and across P (P: the block's first byte): whichever "
                  "block a part starts at, its first markers are rel = -32768, -1 and the first byte that is no marker", blocks, tables)


# ---- six blocks, the fourth one special ------------------------------------------------------------------------------------------

def _ordinary(rng, n):
    """a table of n ordinary tokens; 32 KiB of output lie in front of it"""
    ref = rng.random(n) < 0.1
    run = np.minimum(3 + (rng.geometric(1 / 20, n) - 1), 258)
    dist = np.minimum(1 + (rng.random(n) ** 3 * 32768).astype(np.int64), 32768)
    lit = np.where(ref, -1, rng.integers(0, 256, n))
    return ob.symbol_tokens(lit, np.where(ref, run, 0), np.where(ref, dist, 0))


def _six(seed, special):
    """-> (blocks, tables, rng): 32 KiB of literals, two blocks of 12 000 tokens (more than 50 KB of input), the special block, two
    more ordinary ones.  special(rng) -> ((bytes, bits), token table or None)"""
    rng = np.random.default_rng(seed)
    tables = [_lits(rng.integers(0, 256, HEAD)), _ordinary(rng, 12000), _ordinary(rng, 12000)]
    blocks = [_block(t) for t in tables]
    blk, tab = special(rng)
    tail = [_ordinary(rng, 3000), _ordinary(rng, 3000)]
    return blocks + [blk, _block(tail[0]), _block(tail[1], final=True)], tables + [tab] + tail


def _mixed(rng, n, lsyms, dsyms, lits):
    """n tokens, three in ten of them references: length symbols from lsyms, distance symbols from dsyms, every extra bit random"""
    lx = np.zeros(288, np.int64); lx[257:286] = ob.LEN_EXTRA
    dx = np.zeros(32, np.int64); dx[:30] = ob.DIST_EXTRA
    t = _lits(rng.choice(lits, n))
    ref = rng.random(n) < 0.3
    m = int(ref.sum())
    ls, ds = rng.choice(lsyms, m), rng.choice(dsyms, m)
    t[ref] = np.stack([ls, rng.integers(0, 1 << 30, m) & ((1 << lx[ls]) - 1), ds, rng.integers(0, 1 << 30, m) & ((1 << dx[ds]) - 1)], axis=1)
    return t


def _one_distance(rng):
    t = _lits(rng.integers(0, 256, 1800))
    at = rng.choice(1800, 300, replace=False)
    t[at] = _refs(rng.integers(3, 259, 300), rng.integers(33, 49, 300))          # distance symbol 10 (four extra bits), and no other
    llen, dlen = ob.token_lengths(t, complete=False)
    assert np.count_nonzero(dlen) == 1 and dlen[10] == 1
    return ob.coded_block(llen, dlen, t, final=False), t


def _no_distance(rng):
    t = _lits(rng.integers(0, 256, 2000))
    llen, dlen = ob.token_lengths(t, complete=False)
    assert not dlen.any()
    return ob.coded_block(llen, dlen, t, final=False), t


def deep_lengths():
    """Fibonacci-weighted (one code per depth): literals 0 .. 127 share the upper half with 8 bits each; below it 2, 3, .. 13 bits
    (literals 128 .. 139), 14 (end of block), 15 and 15 (length symbols 284 -- five extra bits -- and 285).  Distance symbols
    14 .. 29: 1, 2, .. 14, 15, 15 bits.  A reference 284 / 29 is 15 + 5 + 15 + 13 = 48 bits, the longest token there is."""
    ll = np.zeros(286, np.int64)
    ll[:128] = 8
    ll[128:140] = np.arange(2, 14)
    ll[256], ll[284], ll[285] = 14, 15, 15
    dl = np.zeros(30, np.int64)
    dl[14:28] = np.arange(1, 15)
    dl[28] = dl[29] = 15
    return ll, dl


def _deep15(rng):
    ll, dl = deep_lengths()
    t = _mixed(rng, 2500, [284, 285], np.arange(14, 30), np.arange(140))
    return ob.coded_block(ll, dl, t, final=False), t


def full_lengths():
    """all 286 literal/length and all 30 distance symbols coded: 226 x 8 + 60 x 9 bits; 9, 9, 8, 7, 6, 5, 4, 3, 4, 4 and 20 x 5 bits.
    The run of nines goes from literal/length symbol 226 through the last one into the first two distance lengths."""
    ll = np.array([8] * 226 + [9] * 60, np.int64)
    dl = np.array([9, 9, 8, 7, 6, 5, 4, 3, 4, 4] + [5] * 20, np.int64)
    return ll, dl


def _full(rng):
    ll, dl = full_lengths()
    t = _mixed(rng, 3000, np.arange(257, 286), np.arange(30), np.arange(256))
    return ob.coded_block(ll, dl, t, final=False, repeats=True, nl=286, nd=30), t


def cl7_lengths():
    """the code-length code 1, 2, .. 7, 7 bits deep over the eight symbols 8, 9, 5, 4, 3, 6, 7 (full_lengths' values, most frequent
    first) and 0, which has a code here and is not used"""
    clen = np.zeros(19, np.int64)
    for sym, n in zip([8, 9, 5, 4, 3, 6, 7, 0], [1, 2, 3, 4, 5, 6, 7, 7]):
        clen[sym] = n
    return clen


def _cl7(rng):
    ll, dl = full_lengths()
    t = _mixed(rng, 3000, np.arange(257, 286), np.arange(30), np.arange(256))
    return ob.coded_block(ll, dl, t, final=False, clen=cl7_lengths()), t


HEADERS = {
    "headers-one-distance": (_one_distance, "one distance code of one bit, used by 300 references"),
    "headers-no-distance": (_no_distance, "no distance code at all: literals only"),
    "headers-deep15": (_deep15, "15-bit codes in the literal/length AND the distance code of one block, the deepest codes used: the "
                       "second-level tables both alphabets share"),
    "headers-full": (_full, "HLIT = 286 and HDIST = 30, the header run-length coded with a repeat code 16 across the HLIT boundary"),
    "headers-cl7": (_cl7, "a code-length code 7 bits deep"),
}


def header_case(name):
    special, purpose = HEADERS[name]
    blocks, tables = _six(200 + sorted(HEADERS).index(name), special)
    return _valid(name, purpose, blocks, tables)


def _reach(name, seed, beyond):
    rng = np.random.default_rng(seed)
    first = _lits(rng.integers(0, 256, 1000))
    second = np.concatenate([_refs([10], [1000 + beyond]), _lits(rng.integers(0, 256, 500))])
    return [_block(first), _block(second, final=True)], [first, second]


def reach_exact():
    return _valid("reach-exact", "the second block's first token reaches back exactly as many bytes as there are (the valid twin of "
                  "reach-beyond)", *_reach("reach-exact", 301, 0))


# ---- the malformed cases ---------------------------------------------------------------------------------------------------------
# What the reference (swift-png's LZ77 inflator) does with each, by the lines of its source that decide it; the oracle
# (oracle/inflate.c) restates these.  Recorded below: the oracle's status, bytes written and error payload.

EXPECT = {
    # (status, bytes written, error payload) as the oracle gave them; tests/test_deflate_cases.py asserts that it still says so
    "ref-without-distance": (67, 109637, (0, 0)),
    "no-end-of-block": (1, 114192, (0, 0)),
    "oversubscribed": (38, 108128, (0, 0)),
    "incomplete-distance": (38, 108733, (0, 0)),
    "fixed-d30": (67, 106083, (0, 0)),
    "fixed-l286": (0, 124392, (0, 0)),
    "reach-beyond": (39, 1000, (0, 0)),
    "periods-capacity": (64, 3076986, (0, 0)),
    "echo-truncated": (1, 438884, (0, 0)),
    "echo-checksum": (32, 884736, (2564522863, 2564522862)),
}


def _ref_without_distance(rng):
    # HuffmanTree.swift:112-135 (validate(symbols:normalizing:): no length above 0 -> init(stub: nil)), :52-65 (the stub has no
    # symbols and size (256, 256): table() writes nothing); InflatorBuffers.Stream.swift:341-342 loads the LZ77.Distance from that
    # uninitialised table.  The oracle marks such entries (len == 0) and reports 67 where the reference reads one.
    t = _lits(rng.integers(0, 256, 600))
    t[300] = (260, 0, 0, 0)                                                      # a run of 6; its distance has no code, so no bits
    llen, _ = ob.token_lengths(t, complete=False)
    return ob.coded_block(llen, np.zeros(1, np.int64), t, final=False), t


def _no_end_of_block(rng):
    # InflatorBuffers.Stream.swift:266-380 (readBlock(with:)): the loop leaves only through symbol 256 (:299-315) or when the input
    # is used up (:268, :284-288 -> nil: more input wanted).  A complete code of the 256 literals has no 256: everything behind the
    # block's tokens -- two blocks and the trailer -- is read as literals, and the answer is 1.  (zlib refuses the table.)
    t = _lits(rng.integers(0, 256, 500))
    return ob.coded_block(np.full(256, 8, np.int64), np.zeros(1, np.int64), t, final=False, eob=False, nl=257), t


def _oversubscribed(rng):
    # HuffmanTree.swift:80-108 (size: interior nodes left over must be 0 -- 257 codes of 8 bits leave -1), :158-162 (validate -> nil),
    # InflatorBuffers.Stream.swift:252-260: invalidHuffmanTable = 38
    return ob.coded_block(np.full(257, 8, np.int64), np.array([1, 1], np.int64), np.zeros((0, 4), np.int64), final=False, eob=False), None


def _incomplete_distance(rng):
    # HuffmanTree.swift:112-135: the second symbol with a length sends the lengths to the ordinary validate(symbols:lengths:), whose
    # size (:80-108) finds an interior node left over for lengths 1 and 2 -> nil; InflatorBuffers.Stream.swift:252-260: 38
    t = _lits(rng.integers(0, 256, 500))
    llen, _ = ob.token_lengths(t, complete=False)
    return ob.coded_block(llen, np.array([1, 2], np.int64), t, final=False), t


def _fixed_with(token):
    def special(rng):
        t = _lits(rng.integers(0, 256, 600))
        t[300] = token
        return ob.fixed_block(t, final=False), t
    return special


MALFORMED = {
    "ref-without-distance": (_ref_without_distance, "a reference in a block without a distance code"),
    "no-end-of-block": (_no_end_of_block, "a table without an end-of-block code"),
    "oversubscribed": (_oversubscribed, "an over-subscribed literal/length code"),
    "incomplete-distance": (_incomplete_distance, "an incomplete distance code of two codes"),
    # Composites.swift:105-110: decades 30 and 31 are padding rows (extra 0, base 0), so distance symbol 30 is offset 0:
    # InflatorBuffers.Stream.swift:358-362 lets it pass (endIndex - 0 >= startIndex) and InflatorOut.swift:133-136 copies each byte
    # from itself, i.e. from memory nobody wrote.  The oracle reports 67 (count > 0 and offset 0).
    "fixed-d30": (_fixed_with((257, 0, 30, 0)), "a fixed block with distance symbol 30"),
    # Composites.swift:61-66: length symbols 286 and 287 are decades 30 and 31 of the run table, padding rows too: a run of 0
    # bytes.  The distance behind it is read as usual (InflatorBuffers.Stream.swift:341-347) and expand(offset:count: 0) copies
    # nothing: for the reference nothing is wrong, the stream goes on and ends well (status 0).  zlib refuses the symbol.
    "fixed-l286": (_fixed_with((286, 0, 0, 0)), "a fixed block with length symbol 286 (the reference: a run of no bytes, and on it goes)"),
}


def malformed_case(name):
    special, purpose = MALFORMED[name]
    blocks, tables = _six(400 + sorted(MALFORMED).index(name), special)
    return _malformed(name, purpose + ", behind 50 KB of good blocks", blocks, tables)


def reach_beyond():
    # InflatorBuffers.Stream.swift:358-362: endIndex - offset < startIndex -> invalidStringReference = 39
    return _malformed("reach-beyond", "the second block's first token reaches one byte in front of the output",
                      *_reach("reach-beyond", 301, 1))


def periods_capacity():
    c = case("periods")
    ref, run, _ = runs_and_distances(c.blocks[0])
    pos = np.cumsum(run) - run
    k = np.nonzero(ref & (run == 258) & (pos > 3_000_000))[0][0]
    cap = int(pos[k]) + 100
    # (no counterpart in the reference, whose output grows: the boundary's SPNG_E_OUTPUT_CAPACITY = 64, nothing of the run written)
    return Case("periods-capacity", c.stream, ZLIB, "periods with an output capacity that ends inside a 258-byte run", False, cap=cap,
                expect=EXPECT.get("periods-capacity"), blocks=c.blocks, info={"run_at": int(pos[k])})


def echo_truncated():
    c = case("echo")
    bits = c.info["block_bits"]
    cut = 2 + (bits[13] + bits[14]) // 16                                        # (block 0 is the literals: the 13th echo block)
    # InflatorBuffers.Stream.swift:349-356: a token the input does not hold completely -> nil: 1, with every byte in front of it
    return Case("echo-truncated", c.stream[:cut], ZLIB, "echo cut off in the middle of its 13th block", False, cap=1 << 20,
                expect=EXPECT.get("echo-truncated"), blocks=c.blocks, info={"cut": cut})


def echo_checksum():
    c = case("echo")
    z = bytearray(c.stream)
    z[-1] ^= 0x01
    # InflatorBuffers.swift:112-130: invalidStreamChecksum(declared:computed:) = 32
    return Case("echo-checksum", bytes(z), ZLIB, "echo with a wrong Adler-32", False, cap=1 << 20, expect=EXPECT.get("echo-checksum"),
                blocks=c.blocks)


BUILDERS = {
    "periods": periods, "extremes": extremes, "dense3": lambda: dense("dense3", 103, False), "dense34": lambda: dense("dense34", 106, True),
    "dense-blocks": dense_blocks, "echo": echo, "edges": edges, "reach-exact": reach_exact,
    **{n: functools.partial(header_case, n) for n in HEADERS},
    **{n: functools.partial(malformed_case, n) for n in MALFORMED},
    "reach-beyond": reach_beyond, "periods-capacity": periods_capacity, "echo-truncated": echo_truncated, "echo-checksum": echo_checksum,
}
NAMES = list(BUILDERS)
VALID = [n for n in NAMES if n in ("periods", "extremes", "dense3", "dense34", "dense-blocks", "echo", "edges", "reach-exact") or n in HEADERS]
INVALID = [n for n in NAMES if n not in VALID]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    c = BUILDERS[name]()
    assert c.name == name and c.valid == (name in VALID)
    return c


def expected(c: Case):
    """what the device must say: the oracle's (status, output bytes, consumed, aux) for the case's stream and capacity"""
    if c.valid:
        data = c.info["data"]
        return ph.orc_inflate(c.stream, c.fmt, cap=len(data) + 64)
    return ph.orc_inflate(c.stream, c.fmt, cap=c.cap)
