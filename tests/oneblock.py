"""Test-side DEFLATE writers for streams that are ONE block (tests/test_emu_blockcuts.py, tests/test_gpu_blockcuts.py): zlib closes a
block every 16-32 K symbols whatever it is asked, so blocks of any size are assembled here, with numpy only.  What they must
inflate to is always asked of zlib (zlib.decompress), never computed here."""
import heapq
import zlib

import numpy as np

# RFC 1951, 3.2.5: base run of length symbols 257 .. 285 and their extra bits; base distance of symbols 0 .. 29 and theirs
LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LEN_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0])
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                      8193, 12289, 16385, 24577])
DIST_EXTRA = np.array([0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)])
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def huffman_lengths(hist, limit):
    """code lengths of a Huffman code for the symbols with hist > 0 (at least two of them); asserts depth <= limit"""
    used = [int(i) for i in np.nonzero(hist)[0]]
    assert len(used) >= 2
    hist = np.asarray(hist, np.int64)
    for _ in range(64):                                   # (too deep: once more with the counts halved, i.e. flattened)
        heap = [(int(hist[i]), i, (i,)) for i in used]
        heapq.heapify(heap)
        lens = np.zeros(len(hist), np.int64)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for i in a[2] + b[2]:
                lens[i] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if lens.max() <= limit:
            break
        hist = np.where(hist > 0, (hist + 1) // 2, 0)
    assert lens.max() <= limit, f"Huffman depth {lens.max()} > {limit}"
    return lens


def canonical_codes(lens):
    """RFC 1951, 3.2.2 -- and turned round: Huffman codes go out most significant bit first, everything else least"""
    codes = np.zeros(len(lens), np.int64)
    code = 0
    for n in range(1, int(lens.max()) + 1):
        for i in np.nonzero(lens == n)[0]:
            codes[i] = int(format(code, f"0{n}b")[::-1], 2)
            code += 1
        code <<= 1
    return codes


def pack_bits(values, nbits):
    """the fields (value, bits), least significant bit first, one after the other -> bytes (repeat / cumsum)"""
    values = np.asarray(values, np.int64)
    nbits = np.asarray(nbits, np.int64)
    keep = nbits > 0
    values, nbits = values[keep], nbits[keep]
    total = int(nbits.sum())
    starts = np.cumsum(nbits) - nbits
    if total > (1 << 26):
        # (a bit per array element is too much for blocks of many MiB: every field, <= 15 bits, shifted to its place in its first
        # byte, is three bytes at most; fields do not overlap, so adding the bytes up is OR-ing them)
        assert int(nbits.max()) <= 16
        out = np.zeros((total + 7) // 8 + 3, np.float64)
        at, val = starts >> 3, values << (starts & 7)
        for k in range(3):
            out += np.bincount(at + k, weights=((val >> (8 * k)) & 255).astype(np.float64), minlength=len(out))
        return out[:(total + 7) // 8].astype(np.uint8).tobytes(), total
    assert total < 2 ** 31 and len(nbits) < 2 ** 31
    field = np.repeat(np.arange(len(nbits), dtype=np.int32), nbits)
    within = np.arange(total, dtype=np.int32) - starts.astype(np.int32)[field]
    bits = ((values.astype(np.int32)[field] >> within) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def random_tokens(seed, out_bytes, match=0.3, mean_run=24, alphabet=64):
    """literals (32 KiB of them first, so that every distance is valid) and (run, distance) pairs from a fixed-seed distribution that
    stand for about out_bytes bytes: -> (literal or -1, run, distance) arrays"""
    rng = np.random.default_rng(seed)
    per = (1 - match) + match * (mean_run + 3)
    n = max(int((out_bytes - 32768) / per), 16)
    is_ref = rng.random(n) < match
    run = 3 + (rng.geometric(1.0 / mean_run, n) - 1) % 120           # (no rare long runs: the code stays below 16 bits)
    dist = np.minimum(1 + (rng.random(n) ** 3 * 32768).astype(np.int64), 32768)
    lit = np.where(rng.random(n) < 0.5, (rng.geometric(0.08, n) - 1) % alphabet, rng.integers(0, 256, n))
    head = rng.integers(0, 256, 32768)
    lit = np.concatenate([head, np.where(is_ref, -1, lit)])
    z = np.zeros(32768, np.int64)
    return lit.astype(np.int64), np.concatenate([z, np.where(is_ref, run, 0)]), np.concatenate([z, np.where(is_ref, dist, 0)])


def dynamic_block(lit, run, dist, final=True):
    """ONE dynamic-Huffman block of these tokens -> (bytes, bits): raw DEFLATE, not padded beyond its last byte"""
    is_ref = lit < 0
    ls = np.searchsorted(LEN_BASE, run[is_ref], side="right") - 1
    ds = np.searchsorted(DIST_BASE, dist[is_ref], side="right") - 1
    sym = lit.copy()
    sym[is_ref] = 257 + ls
    lhist = np.bincount(np.concatenate([sym, [256]]), minlength=286)
    dhist = np.bincount(ds, minlength=30)
    if np.count_nonzero(dhist) < 2:                       # (a complete distance code)
        dhist[:2] += 1
    llen, dlen = huffman_lengths(lhist, 15), huffman_lengths(dhist, 15)
    lcode, dcode = canonical_codes(llen), canonical_codes(dlen)
    nl = max(257, int(np.nonzero(llen)[0].max()) + 1)
    nd = max(1, int(np.nonzero(dlen)[0].max()) + 1)
    # the header: the code lengths one symbol each (no repeat codes), themselves Huffman-coded
    seq = np.concatenate([llen[:nl], dlen[:nd]])
    clen = huffman_lengths(np.bincount(seq, minlength=19), 7)
    ccode = canonical_codes(clen)
    ncl = max(4, max(i for i, s in enumerate(CL_ORDER) if clen[s]) + 1)
    hv = [1 if final else 0, 2, nl - 257, nd - 1, ncl - 4] + [int(clen[s]) for s in CL_ORDER[:ncl]] + [int(c) for c in ccode[seq]]
    hn = [1, 2, 5, 5, 4] + [3] * ncl + [int(c) for c in clen[seq]]
    # the tokens: four fields each (code, run's extra bits, distance code, its extra bits); literals leave three empty
    n = len(sym)
    v = np.zeros((n + 1, 4), np.int64)
    b = np.zeros((n + 1, 4), np.int64)
    v[:n, 0], b[:n, 0] = lcode[sym], llen[sym]
    idx = np.nonzero(is_ref)[0]
    v[idx, 1], b[idx, 1] = run[is_ref] - LEN_BASE[ls], LEN_EXTRA[ls]
    v[idx, 2], b[idx, 2] = dcode[ds], dlen[ds]
    v[idx, 3], b[idx, 3] = dist[is_ref] - DIST_BASE[ds], DIST_EXTRA[ds]
    v[n, 0], b[n, 0] = lcode[256], llen[256]
    return pack_bits(np.concatenate([hv, v.reshape(-1)]), np.concatenate([hn, b.reshape(-1)]))


def one_dynamic_block(seed, out_bytes, **kw):
    """a zlib stream that is one final dynamic block -> (expected bytes, stream)"""
    body, _ = dynamic_block(*random_tokens(seed, out_bytes, **kw))
    data = zlib.decompressobj(-15).decompress(body)
    return data, b"\x78\x01" + body + zlib.adler32(data).to_bytes(4, "big")


def literal_block(data):
    """one final dynamic block of these bytes as literals (an fpnge-shaped stream: the whole image in one block)"""
    a = np.frombuffer(data, np.uint8).astype(np.int64)
    body, _ = dynamic_block(a, np.zeros(len(a), np.int64), np.zeros(len(a), np.int64))
    return b"\x78\x01" + body + zlib.adler32(data).to_bytes(4, "big")


def one_fixed_block(seed, n):
    """a zlib stream that is one final fixed-Huffman block of n literals below 144 (eight bits each, most significant first) and
    the end-of-block code -> (expected bytes, stream)"""
    vals = np.random.default_rng(seed).integers(0, 144, n, dtype=np.uint8)
    bits = np.concatenate([np.array([1, 1, 0], np.uint8), np.unpackbits((vals + 0x30)[:, None], axis=1, bitorder="big").reshape(-1),
                           np.zeros(7, np.uint8)])
    data = vals.tobytes()
    return data, b"\x78\x01" + np.packbits(bits, bitorder="little").tobytes() + zlib.adler32(data).to_bytes(4, "big")


def dynamic_then_fixed(seed, n_dynamic, n_fixed):
    """a dynamic block and, behind it, one long fixed block that no search finds a header in: the segments behind the first lie in a
    block with other tables than their anchor's -> (expected bytes, stream)"""
    head, hbits = dynamic_block(*random_tokens(seed, n_dynamic), final=False)
    vals = np.random.default_rng(seed + 1).integers(0, 144, n_fixed, dtype=np.uint8)
    hb = np.unpackbits(np.frombuffer(head, np.uint8), bitorder="little")[:hbits]
    bits = np.concatenate([hb, np.array([1, 1, 0], np.uint8), np.unpackbits((vals + 0x30)[:, None], axis=1, bitorder="big").reshape(-1),
                           np.zeros(7, np.uint8)])
    body = np.packbits(bits, bitorder="little").tobytes()
    data = zlib.decompressobj(-15).decompress(body)
    return data, b"\x78\x01" + body + zlib.adler32(data).to_bytes(4, "big")
