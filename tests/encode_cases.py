"""Inputs that put every rule of the match finder and of the greedy / lazy parse on its boundary: the encoder's counterpart of
tests/deflate_cases.py, shared by the CPU proof and the emulator runs (tests/test_encode_cases.py) and the GPU parity tests
(tests/test_gpu_encode_cases.py).  Importable without a GPU; nothing is read from disk.

The rules are those of LZ77.DeflatorWindow.match (LZ77.DeflatorWindow.swift:78-212) and of Stream.compress
(DeflatorBuffers.Stream.swift:64-404); the device restates them with 13-bit bucket chains that hold foreign keys, 16-bit heads
swept every 2^14 positions and a ring re-warmed at every chunk start (d3_search_chunk, d3_insert, d3_insert_quad,
dfl4_walk_kernel in csrc/deflate.hip).  What a compressor makes of noise, runs and text only meets such a boundary by chance.
Here a case PLANTS snippets in seeded random filler and states, per level, the exact list of match tokens
(position, run, distance) the planted bytes must produce -- everything else in the stream must be literals, which is also what
shows that the filler added no match of its own.  The proof is in the oracle's own tokens, read back by tests/deflate_tokens.py.

    NAMES, case(name) -> Case(name, data, exponent, levels, purpose, expect, blocks, empty)
    expect[level]   the match tokens, in order
    blocks[level]   {block index: term count} where the case speaks about blocks
    empty           True where the point of the case is that NO match is written (at some level)

A match is only ever written for a run > 5 (DeflatorWindow.swift:115-130), so a repeat of four or five bytes is a candidate that
costs an attempt and leaves no token."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

ALL = (0, 1, 2, 3, 4, 5, 6, 7)
ATTEMPTS = (1, 2, 4, 40, 20, 40, 64, 100)            # LZ77.DeflatorSearch.swift:17-25
GOAL = (6, 8, 10, 24, 32, 54, 80, 160)
LAZY = (False, False, False, False, True, True, True, True)
HBITS = 13                                           # SPNG_D3_HBITS


@dataclass(frozen=True)
class Case:
    name: str
    data: bytes
    exponent: int
    levels: tuple
    purpose: str
    expect: dict = field(hash=False, compare=False)
    blocks: dict = field(default_factory=dict, hash=False, compare=False)
    empty: bool = False
    places: dict = field(default_factory=dict, hash=False, compare=False)    # {level: positions of the planted tokens} where they are not the last ones


def bucket(key4: bytes) -> int:
    """the device's bucket of a position: (little-endian dword * 0x9E3779B1) >> 19 (d3_insert)"""
    return ((int.from_bytes(key4, "little") * 0x9E3779B1) & 0xffffffff) >> (32 - HBITS)


def other(*vals):
    """a byte value none of `vals` has"""
    return next(v for v in range(255, -1, -1) if v not in vals)


class Plan:
    """seeded random filler with planted pieces; pieces and their guard bytes never overlap"""

    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        self.used = np.zeros(n, bool)
        self.guards = 0

    def snippet(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def put(self, pos, piece, before=None, after=None):
        """piece at pos; before / after: the byte in front of it / behind it must not be one of these values"""
        lo, hi = pos - (before is not None and pos > 0), pos + len(piece) + (after is not None)
        assert 0 <= lo and hi <= len(self.b), (pos, len(piece), len(self.b))
        assert not self.used[lo:hi].any(), ("pieces overlap", pos)
        self.used[lo:hi] = True
        self.b[pos:pos + len(piece)] = piece
        if before is not None and pos > 0:
            self.b[pos - 1] = self.guard(before)
        if after is not None:
            self.b[pos + len(piece)] = self.guard(after)
        return pos

    def guard(self, avoid):
        """a byte value that is none of `avoid` and that no guard of this plan has had (two copies never agree one byte further)"""
        while True:
            v = (0xa5 + 0x3b * self.guards) & 0xff
            self.guards += 1
            assert self.guards < 250
            if v not in avoid:
                return v

    def copies(self, piece, *positions):
        """the same piece several times: the bytes in front of the copies differ from each other, and so do the bytes behind"""
        for k, pos in enumerate(positions):
            self.put(pos, piece, before=(), after=())
            if pos > 0:
                self.b[pos - 1] = (0x11 + 0x25 * k) & 0xff
            self.b[pos + len(piece)] = (0x23 + 0x3b * k) & 0xff

    def bytes(self):
        return bytes(self.b)


def _same(levels, tokens):
    return {lv: list(tokens) for lv in levels}


# ---- the window's far edge -----------------------------------------------------------------------------------------------------

def edge(e, tag):
    off = {"m2": -2, "m1": -1, "0": 0, "p1": 1}[tag]
    d, x = (1 << e) + off, 3000
    p = Plan(1000 + 10 * e + off, x + d + 300)
    p.copies(p.snippet(16), x, x + d)
    found = d <= (1 << e) - 1
    return Case(f"edge-e{e}-{tag}", p.bytes(), e, ALL, f"a first candidate at distance 2^{e} {off:+d} is " + ("taken" if found else "out of the window")
                + " (acc > wmask; the oracle removes the head 2^e back before it looks)", _same(ALL, [(x + d, 16, d)] if found else []), empty=not found)


def second(e, tag):
    mask = (1 << e) - 1
    g, x = mask - (tag == "m1"), 3000
    p = Plan(1100 + 10 * e + (tag == "m1"), x + g + 300)
    P, Q, R = p.snippet(6), p.snippet(10), p.snippet(10)
    R = bytes([other(Q[0])]) + R[1:]
    p.copies(P + Q, x, x + g)
    p.put(x + g - 50, P + R, before=(P[0],), after=())
    mid = (x + g - 50, 6, g - 50)
    split = [mid, (x + g, 6, 50), (x + g + 6, 10, g)]           # the nearer P alone, then Q from the older copy as ITS first candidate
    whole = [mid, (x + g, 16, g)]
    expect = {lv: split if lv == 0 or g == mask else whole for lv in ALL}
    return Case(f"second-e{e}-{tag}", p.bytes(), e, ALL, f"P+Q, P+R 50 in front of the second P+Q at distance 2^{e} - 1{' - 1' if tag == 'm1' else ''}: a candidate "
                "behind the first is refused at distance == mask (distance < mask), taken one nearer; level 0 never asks for it", expect)


# ---- bucket chains -------------------------------------------------------------------------------------------------------------

def _foreign(key, count, seed):
    """`count` different keys of the bucket of `key`, none equal to it"""
    rng, out, h = np.random.default_rng(seed), [], bucket(key)
    while len(out) < count:
        c = rng.integers(0, 256, (1 << 16, 4), dtype=np.uint8)
        k = c[:, 0].astype(np.uint64) | c[:, 1].astype(np.uint64) << 8 | c[:, 2].astype(np.uint64) << 16 | c[:, 3].astype(np.uint64) << 24
        hit = np.nonzero(((k * 0x9E3779B1) & 0xffffffff) >> (32 - HBITS) == h)[0]
        for i in hit:
            f = c[i].tobytes()
            if f != key and f not in out and len(out) < count:
                out.append(f)
    for f in out:
        assert bucket(f) == h and f != key
    assert len(set(out)) == count
    return out


def bucket_foreign():
    x = 2000
    p = Plan(1200, 4000)
    S = p.snippet(16)
    p.copies(S, x, x + 400)
    F = _foreign(S[:4], 5, 1201)
    for j, f in enumerate(F):
        p.put(x + 100 + 40 * j, f, before=(), after=())
    assert len({bucket(S[:4])} | {bucket(f) for f in F}) == 1 and len({S[:4], *F}) == 6
    return Case("bucket-foreign", p.bytes(), 15, ALL, "five other keys of the snippet's 13-bit bucket between its two copies: the walk skips them "
                "without spending the attempt (level 0 has one)", _same(ALL, [(x + 400, 16, 400)]))


def bucket_same_batch():
    B = 4096                                                   # batches are 64 aligned positions, quads 256
    p = Plan(1210, 8192)
    low, high = [], []                                         # tokens of level 0 / of levels 1-7
    S1 = p.snippet(16)                                         # two positions of one key in a batch
    p.copies(S1, B + 5, B + 30)
    low += [(B + 30, 16, 25)]; high += [(B + 30, 16, 25)]

    def pqr(first, mid, last):                                 # P+Q, P+R, P+Q: the chain's ORDER shows in the tokens
        P, Q, R = p.snippet(6), p.snippet(10), p.snippet(10)
        R = bytes([other(Q[0])]) + R[1:]
        p.copies(P + Q, first, last)
        p.put(mid, P + R, before=(P[0],), after=())
        lo = [(mid, 6, mid - first), (last, 6, last - mid), (last + 6, 10, last - first)]
        hi = [(mid, 6, mid - first), (last, 16, last - first)]
        return lo, hi

    def fgn(first, last, *between):                            # the same key with foreign keys of its bucket between
        S = p.snippet(16)
        p.copies(S, first, last)
        for at, f in zip(between, _foreign(S[:4], len(between), first)):
            p.put(at, f, before=(), after=())
        return [(last, 16, last - first)]

    lo, hi = pqr(B + 256 + 5, B + 256 + 25, B + 256 + 45); low += lo; high += hi       # three positions of one key in a batch
    t = fgn(B + 512 + 5, B + 512 + 45, B + 512 + 25, B + 512 + 35); low += t; high += t
    lo, hi = pqr(B + 1024 + 10, B + 1024 + 80, B + 1024 + 160); low += lo; high += hi  # ... in three batches of one quad
    t = fgn(B + 1536 + 10, B + 1536 + 200, B + 1536 + 100, B + 1536 + 130); low += t; high += t
    return Case("bucket-same-batch", p.bytes(), 15, ALL, "two and three positions of one bucket -- the same key, and foreign keys -- inside one batch of 64 "
                "positions and inside one quad of 256: what the one-exchange inserter and the read-back inserter order",
                {lv: low if lv == 0 else high for lv in ALL})


# ---- attempts and goal ---------------------------------------------------------------------------------------------------------

ATTEMPT_NS = tuple(sorted({a - 1 for a in ATTEMPTS} | set(ATTEMPTS)))


def attempts(n):
    x = 2000
    p = Plan(1300 + n, 6000)
    K, Q = p.snippet(4), p.snippet(12)
    last = x + 24 + 8 * n + 8
    p.copies(K + Q, x, last)
    g = [v for v in range(256) if v != Q[0]]
    for j in range(n):                                         # K and a fifth byte of its own: a run of 4, a candidate and no token
        p.put(x + 24 + 8 * j, K + bytes([g[j]]))
    d = last - x
    assert d < 32767                                           # every candidate inside the window
    expect = {lv: [(last, 16, d)] if n < ATTEMPTS[lv] else [(last + 1, 15, d)] for lv in ALL}
    return Case(f"attempts-{n}", p.bytes(), 15, ALL, f"a run of 16 behind {n} candidates of the same key with runs of 4: found iff {n} < attempts "
                "(rem > 0), else one position later where the key is its own", expect)


GOAL_RS = tuple(sorted({g - 1 for g in GOAL} | set(GOAL)))


def goal(r):
    x, y, last = 2000, 2300, 2600
    p = Plan(1400 + r, 4000)
    T = p.snippet(200)
    p.copies(T, x, last)
    p.put(y, T[:r], before=(T[0],), after=(T[r],))
    near = [(y, r, y - x)] if r > 5 else []
    expect = {}
    for lv in ALL:
        on = ATTEMPTS[lv] > 1 and GOAL[lv] > r                 # the walk goes on behind the nearer candidate
        if on:
            t = [(last, 200, last - x)]
        elif LAZY[lv] and r == GOAL[lv]:                       # one position later the nearer run is goal - 1: the walk reaches the older copy, 199 > r
            t = [(last + 1, 199, last - x)]
        elif r > 5:
            t = [(last, r, last - y), (last + r, 200 - r, last - x)]
        else:                                                  # level 0, r = 5: no token for 5, the nearer copy's key at + 1 too, the older copy's from + 2
            t = [(last + 2, 198, last - x)]
        expect[lv] = near + t
    return Case(f"goal-{r}", p.bytes(), 15, ALL, f"a nearer run of {r} in front of an older run of 200: the walk stops iff goal <= {r} (goal > run)", expect)


def equal(r):
    x = 2000
    p = Plan(1450 + r, 4000)
    p.copies(p.snippet(r), x, x + 100, x + 300)
    return Case(f"equal-{r}", p.bytes(), 15, ALL, f"three copies of {r} bytes: the third sees two candidates with the same run and keeps the nearer one (only a "
                "strictly longer run replaces the best, ext < run), whether the walk stops at the first (goal) or goes on", _same(ALL, [(x + 100, r, 100), (x + 300, r, 200)]))


# ---- the lazy rule -------------------------------------------------------------------------------------------------------------

def _lazy_plan(seed, n):
    p = Plan(seed, n)
    return p, p.snippet(16)


def lazy_tie():
    x, last = 2000, 2300
    p, T = _lazy_plan(1500, 4000)
    p.put(x, T[:10], before=(), after=(T[10],))
    p.put(x + 100, T[1:11], before=(T[0],), after=(T[11],))
    p.put(last, T[:11], before=(), after=(T[11],))
    return Case("lazy-tie", p.bytes(), 15, ALL, "a run of 10 and, one position later, a run of 10: the early one stays at every level (erun < lrun is strict)",
                _same(ALL, [(x + 100, 9, 99), (last, 10, last - x)]))


def lazy_win():
    x, last = 2000, 2300
    p, T = _lazy_plan(1501, 4000)
    p.put(x, T[:10], before=(), after=(T[10],))
    p.put(x + 100, T[1:12], before=(T[0],), after=(T[12],))
    p.put(last, T[:12], before=(), after=(T[12],))
    src = [(x + 100, 9, 99)]                                  # (T[1:] at x + 100 against T[1:] at x + 1)
    return Case("lazy-win", p.bytes(), 15, ALL, "a run of 10 and, one position later, a run of 11: a literal and the later run at levels 4-7, the early run at 0-3",
                {lv: src + ([(last + 1, 11, last + 1 - (x + 100))] if LAZY[lv] else [(last, 10, last - x)]) for lv in ALL})


def lazy_chain():
    x, last = 2000, 2500
    p, T = _lazy_plan(1502, 4000)
    p.put(x, T[:10], before=(), after=(T[10],))
    p.put(x + 100, T[1:12], before=(T[0],), after=(T[12],))
    p.put(x + 200, T[2:14], before=(T[1],), after=(T[14],))
    p.put(x + 300, T[3:16], before=(T[2],), after=())
    p.put(last, T, before=(), after=(p.b[x + 300 + 13],))
    src = [(x + 100, 9, 99), (x + 200, 10, 99), (x + 300, 11, 99)]
    lazy = src + [(last + 1, 11, last + 1 - (x + 100))]        # ONE deferral: the longer runs at + 2 and + 3 are never looked at
    greedy = src + [(last, 10, last - x), (last + 10, 6, last + 10 - (x + 300 + 7))]
    return Case("lazy-chain", p.bytes(), 15, ALL, "runs of 10, 11, 12, 13 at four positions in a row: the parse defers once (literal, run 11) and does not look "
                "further; greedy takes 10 and then the 6 that is left", {lv: lazy if LAZY[lv] else greedy for lv in ALL})


# ---- the input's end -----------------------------------------------------------------------------------------------------------

TAIL_RUNS = (258, 259, 260, 261, 262, 263, 520)


def tail_run(n):
    f = 1000
    p = Plan(1600 + n, f)
    c = other(p.b[-1])
    t = [(f + 1, min(n - 1, 258), 1)] + ([(f + 259, 258, 1)] if n == 520 else [])
    return Case(f"tail-run-{n}", p.bytes() + bytes([c]) * n, 15, ALL, f"{n} equal bytes at the end: a literal, runs at distance 1 capped at 258 and by the "
                "input's end, literals for what is left (the last three positions start nothing; four bytes left are a run of 4)", _same(ALL, t))


def tail_end(k):
    n = 1000
    p = Plan(1610 + k, n)
    S = p.snippet(16)
    p.put(500, S, before=(), after=())
    p.put(n - 16 - k, S, before=(p.b[499],), after=(p.b[516],) if k else None)
    return Case(f"tail-end-{k}", p.bytes(), 15, ALL, f"a snippet of 16 whose second copy ends {k} bytes in front of the input's end", _same(ALL, [(n - 16 - k, 16, n - 16 - k - 500)]))


def tail_cut(m):
    n = 1000
    p = Plan(1620 + m, n)
    S = p.snippet(16)
    p.put(500, S, before=(), after=())
    p.put(n - m, S[:m], before=(p.b[499],), after=None)
    t = [(n - m, m, n - m - 500)] if m > 5 else []
    return Case(f"tail-cut-{m}", p.bytes(), 15, ALL, f"the input ends {m} bytes into the second copy: the run is cut at the end (lim), " + ("a token" if m > 5 else "5 is no token"),
                _same(ALL, t), empty=m <= 5)


def tail_tiny(n):
    t = [(1, n - 1, 1)] if n >= 7 else []
    return Case(f"tail-tiny-{n}", b"\x07" * n, 15, ALL, f"{n} equal bytes are the whole input: " + ("a literal and a run" if t else "literals only, the run at position 1 is cut below 6"),
                _same(ALL, t), empty=not t)


# ---- ages at which a 16-bit head would alias; sweeps; chunk starts --------------------------------------------------------------

FAR_GAPS = (32768, 32769, 49151, 49152, 65535, 65536, 65537, 98303, 131077)
FAR_LEVELS = (0, 3, 6)


def far_gap(g):
    x = 1000
    p = Plan(1700 + g % 997, x + g + 400)
    p.copies(p.snippet(16), x, x + g)
    c = x + g + 100                                            # the control: the window works right behind the place
    p.copies(p.snippet(16), c - 32767, c)
    return Case(f"far-gap-{g}", p.bytes(), 15, FAR_LEVELS, f"a snippet repeated {g} positions later is not found (a head of that age must not read as a young one); "
                "a control 100 behind it at distance 32767 is", _same(FAR_LEVELS, [(c, 16, 32767)]))


def far_sweep(tag):
    s = 49152                                                  # a sweep position of a stream alone: chunks of 32768, warm-up starts on multiples of 32768
    q = s - 1 if tag == "front" else s
    p = Plan(1750 + (tag == "front"), s + 400)
    p.copies(p.snippet(16), q - 32767, q)
    return Case(f"far-sweep-{tag}", p.bytes(), 15, FAR_LEVELS, f"a snippet at distance 32767 whose second copy sits just {'in front of' if tag == 'front' else 'behind'} a sweep of "
                "the heads (age 32767 stays, 32768 goes)", _same(FAR_LEVELS, [(q, 16, 32767)]))


CHUNK_CS = (32768, 65536, 40384)                               # chunk starts of a stream alone (twice) and of a five-stream batch


def chunk_edge(c, tag):
    q = c + {"m1": -1, "0": 0, "p1": 1}[tag]
    p = Plan(1800 + c % 991 + q % 7, q + 400)
    p.copies(p.snippet(16), q - 32767, q)
    p.copies(p.snippet(16), q + 40 - 32766, q + 40)
    p.copies(p.snippet(16), q + 80 - 32768, q + 80)
    return Case(f"chunk-edge-{c}-{tag}", p.bytes(), 15, FAR_LEVELS, f"second copies at {c} {q - c:+d} (a chunk start: the window is re-warmed from 32768 in front of it, rounded "
                "down to 256), + 40 and + 80 with their first copies 32767, 32766 and 32768 back: the first two are found", _same(FAR_LEVELS, [(q, 16, 32767), (q + 40, 16, 32766)]))


# ---- block ends ----------------------------------------------------------------------------------------------------------------

BLOCK_LEVELS = (0, 6)
TAILN = 500                                                    # literals behind the planted place


def block_edge(tag):
    """Blocks close in front of a step when 2047 terms are queued (greedy) or 2046 / 2047 (lazy: a step may queue two),
    DeflatorBuffers.Stream.swift:219, 277.  Before the planted place every byte is a literal but for the planted sources."""
    if tag in ("last", "first", "final"):
        at = {"last": 2046, "first": 2047, "final": 2047}[tag]    # literals (= terms) in front of the match
        n = at + 16 + (0 if tag == "final" else TAILN)
        p = Plan(1900 + at + (tag == "final"), n)
        S = p.snippet(16)
        p.put(100, S, before=(), after=())
        p.put(at, S, before=(p.b[99],), after=None if tag == "final" else (p.b[116],))
        rest = 0 if tag == "final" else TAILN
        blocks = {0: {0: 2047, 1: (at - 2047) + 1 + rest} if at == 2047 else {0: 2047, 1: rest},
                  6: {0: 2046, 1: (at - 2046) + 1 + rest}}
        purpose = {"last": "a greedy match is the 2047th term, the last of its block; lazy: the block closed at 2046 and it is the next one's first",
                   "first": "a greedy match is the 2048th term, the first of the second block; lazy: the second of the second block",
                   "final": "the final block is one match that ends at the input's end (lazy: a literal and that match)"}[tag]
        return Case(f"block-edge-{tag}", p.bytes(), 15, BLOCK_LEVELS, purpose, _same(BLOCK_LEVELS, [(at, 16, at - 100)]), blocks)
    # the pair of lazy-win: its source B is a match of 9 itself, eight terms fewer than positions in front of the place
    before = {"pair-in": 2045, "pair-out": 2046}[tag]
    at = before + 8
    p = Plan(1950 + before, at + 12 + TAILN)
    T = p.snippet(16)
    p.put(100, T[:10], before=(), after=(T[10],))
    p.put(300, T[1:12], before=(T[0],), after=(T[12],))
    p.put(at, T[:12], before=(), after=(T[12],))
    expect = {0: [(300, 9, 199), (at, 10, at - 100)], 6: [(300, 9, 199), (at + 1, 11, at + 1 - 300)]}
    # greedy: the match is term before + 1, then the two bytes the run of 10 leaves and the tail
    blocks = {0: {0: 2047, 1: before + 1 + 2 + TAILN - 2047},
              6: {0: 2047, 1: TAILN} if tag == "pair-in" else {0: 2046, 1: 2 + TAILN}}
    purpose = ("a lazy literal-and-match pair becomes terms 2046 and 2047: the block closes at 2047" if tag == "pair-in" else
               "a lazy pair that would become terms 2047 and 2048: the block closes at 2046 in front of it")
    return Case(f"block-edge-{tag}", p.bytes(), 15, BLOCK_LEVELS, purpose, expect, blocks)


DENSE_LEVELS = (0, 3)


def dense_block():
    """17 blocks of 2047 literals, ONE block of 2047 matches and no literal, a block of literals.  Match i copies from d_i back with
    d_0 = 32767 and d_i falling: the source pointer only ever skips FORWARD, so the key at a match's first byte has no younger
    occurrence than its source (older ones lie two generations back, out of the window), and the skip is chosen so that the byte
    behind the source differs from the byte that follows in the data: the run is exactly r_i."""
    front, terms = 17 * 2047, 2047
    rng = np.random.default_rng(2000)
    b = bytearray(rng.integers(0, 256, front, dtype=np.uint8).tobytes())
    runs = list(range(131, 258)) + [131] * (terms - 127)
    tokens, d = [], 32767
    for i, r in enumerate(runs):
        at = len(b)
        s = at - d
        b += b[s:s + r]
        tokens.append((at, r, d))
        if i + 1 < terms:
            skip = 4 if i < 1900 else 1
            while b[s + r + skip] == b[s + r]:                 # (the next match starts with b[s + r + skip])
                skip += 1
            d -= skip
    assert 24577 <= d and all(24577 <= t[2] <= 32767 and 131 <= t[1] <= 257 for t in tokens)
    s_end = tokens[-1][0] - tokens[-1][2] + tokens[-1][1]
    tail = bytearray(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
    tail[0] = other(b[s_end])
    b += tail
    blocks = {17: 2047, 16: 2047, 18: 300}
    return Case("dense-block", bytes(b), 15, DENSE_LEVELS, "one block of 2047 match terms and no literal, distances 24577...32767 and runs 131...257 (13 and 5 extra bits), "
                "between blocks of literals only: the most bits next to the fewest in dfl4_scan / dfl4_place", _same(DENSE_LEVELS, tokens),
                {lv: blocks for lv in DENSE_LEVELS})


# ---- the round boundary --------------------------------------------------------------------------------------------------------

ROUND_LEVELS = (0, 6)
ROUND_VARIANTS = ("pair", "straddle", "first")
ZONE, ZONE_R = 36000, 34000                                    # a zone of noise with the plants; the round boundary lies ZONE_R into it
UNIT_RUNS = 6                                                  # filler unit: a byte 1 + 6 x 258 times (a literal, six runs of 258), four marker bytes


def _round_zone(variant):
    """-> (bytes, {level: tokens relative to the zone's start}).  R: the first position of the next round.
    pair: the lazy-win pair with its early run at R - 1, the round's last position, and its later run at R, the position behind
    the round that a lazy parse looks at; straddle: a run over R - 8 ... R + 7; first: a run at R whose source lies 32767 back."""
    p, R = Plan(2100 + ROUND_VARIANTS.index(variant), ZONE), ZONE_R
    if variant == "pair":
        T = p.snippet(16)
        p.put(R - 2001, T[:10], before=(), after=(T[10],))
        p.put(R - 1001, T[1:12], before=(T[0],), after=(T[12],))
        p.put(R - 1, T[:12], before=(), after=(T[12],))
        return p.bytes(), {0: [(R - 1001, 9, 999), (R - 1, 10, 2000)], 6: [(R - 1001, 9, 999), (R, 11, 1001)]}
    if variant == "straddle":
        p.copies(p.snippet(16), R - 1008, R - 8)
        return p.bytes(), _same(ROUND_LEVELS, [(R - 8, 16, 1000)])
    p.copies(p.snippet(16), R - 32767, R)
    return p.bytes(), _same(ROUND_LEVELS, [(R, 16, 32767)])


def round_small(variant, boundary=3 << 14):
    """the plants around a boundary of the emulator's rounds of 2^14 positions, in noise (not in NAMES: the device has no such rounds)"""
    zone, rel = _round_zone(variant)
    pad = boundary - ZONE_R
    data = np.random.default_rng(2110).integers(0, 256, pad, dtype=np.uint8).tobytes() + zone
    return Case(f"round-small-{variant}", data, 15, ROUND_LEVELS, f"the {variant} plant at a boundary of rounds of 2^14 positions",
                {lv: [(a + pad, r, d) for a, r, d in rel[lv]] for lv in ROUND_LEVELS})


def round_edge(variant):
    """The full-size twin: the same zone with its boundary at 2^21, the device's round.  The filler is runs of one byte between
    unique markers -- unit i is byte i % 256 repeated 1 + 6 x 258 times (a literal and six runs of 258 at distance 1; the same
    byte comes back 256 units = 397 KB later, out of the window) and a marker of four bytes that hold i -- so the stream has some
    fifty thousand tokens, the plain reader takes a second and the token list stays exact."""
    zone, rel = _round_zone(variant)
    R, unit = 1 << 21, 1 + 258 * UNIT_RUNS + 4
    z0 = R - ZONE_R
    out, tokens, i = bytearray(np.random.default_rng(2120).integers(0, 256, z0 % unit, dtype=np.uint8).tobytes()), [], 0

    def units(count):
        nonlocal i
        for _ in range(count):
            at = len(out)
            out.extend(bytes([i % 256]) * (1 + 258 * UNIT_RUNS) + bytes([0xf0 | (i >> 12) & 15, 0x80 | (i >> 8) & 15, (i >> 4) & 15 | 0x40, i & 15 | 0x20]))
            tokens.extend((at + 1 + 258 * j, 258, 1) for j in range(UNIT_RUNS))
            i += 1

    units(z0 // unit)
    assert len(out) == z0
    out += zone
    head, mark = len(tokens), len(out)
    units(20)
    expect = {lv: tokens[:head] + [(a + z0, r, d) for a, r, d in rel[lv]] + tokens[head:] for lv in ROUND_LEVELS}
    assert mark == z0 + ZONE
    return Case(f"round-edge-{variant}", bytes(out), 15, ROUND_LEVELS, f"the {variant} plant at position 2^21, where the device's second round begins: "
                + {"pair": "the early run at the round's last position, the later run at the one behind it that only a lazy parse looks at",
                   "straddle": "a run of 16 over the boundary", "first": "a run at the next round's first position, its source 32767 back"}[variant],
                expect, places={lv: tuple(a + z0 for a, _, _ in rel[lv][-1:]) for lv in ROUND_LEVELS})


_BUILD = {}


def _register():
    for e in (8, 11, 15):
        for tag in ("m2", "m1", "0", "p1"):
            _BUILD[f"edge-e{e}-{tag}"] = functools.partial(edge, e, tag)
        for tag in ("m1", "0"):
            _BUILD[f"second-e{e}-{tag}"] = functools.partial(second, e, tag)
    _BUILD["bucket-foreign"] = bucket_foreign
    _BUILD["bucket-same-batch"] = bucket_same_batch
    for n in ATTEMPT_NS:
        _BUILD[f"attempts-{n}"] = functools.partial(attempts, n)
    for r in GOAL_RS:
        _BUILD[f"goal-{r}"] = functools.partial(goal, r)
    for r in (7, 40):
        _BUILD[f"equal-{r}"] = functools.partial(equal, r)
    _BUILD["lazy-tie"], _BUILD["lazy-win"], _BUILD["lazy-chain"] = lazy_tie, lazy_win, lazy_chain
    for n in TAIL_RUNS:
        _BUILD[f"tail-run-{n}"] = functools.partial(tail_run, n)
    for k in (0, 1, 2, 3):
        _BUILD[f"tail-end-{k}"] = functools.partial(tail_end, k)
    for m in (5, 6, 8):
        _BUILD[f"tail-cut-{m}"] = functools.partial(tail_cut, m)
    for n in range(3, 10):
        _BUILD[f"tail-tiny-{n}"] = functools.partial(tail_tiny, n)
    for g in FAR_GAPS:
        _BUILD[f"far-gap-{g}"] = functools.partial(far_gap, g)
    for tag in ("front", "behind"):
        _BUILD[f"far-sweep-{tag}"] = functools.partial(far_sweep, tag)
    for c in CHUNK_CS:
        for tag in ("m1", "0", "p1"):
            _BUILD[f"chunk-edge-{c}-{tag}"] = functools.partial(chunk_edge, c, tag)
    for tag in ("last", "first", "pair-in", "pair-out", "final"):
        _BUILD[f"block-edge-{tag}"] = functools.partial(block_edge, tag)
    _BUILD["dense-block"] = dense_block
    for v in ROUND_VARIANTS:
        _BUILD[f"round-edge-{v}"] = functools.partial(round_edge, v)


_register()
NAMES = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = _BUILD[name]()
    assert c.name == name and set(c.expect) == set(c.levels)
    return c


def pairs(prefixes=None):
    """every (name, level) of the table, or of the families named"""
    return [(n, lv) for n in NAMES if prefixes is None or n.startswith(tuple(prefixes)) for lv in case(n).levels]


def cuts(c: Case, level: int):
    """where to cut a case that is pushed in pieces: one position before, at and after each planted match, and 258 / 259 positions
    before it (the look-ahead a push that is not the last holds back)"""
    out = set()
    for pos in c.places.get(level) or [t[0] for t in c.expect[level][-2:]]:     # (the last tokens are the planted place, in front of them its sources)
        out |= {pos - 259, pos - 258, pos - 1, pos, pos + 1}
    return tuple(sorted(x for x in out if 0 < x < len(c.data)))
