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


def symbol_tokens(lit, run, dist):
    """(literal or -1, run, distance) arrays -> the token table of coded_block: a row (literal/length symbol, the run's extra bits,
    distance symbol or -1, the distance's extra bits) per token"""
    lit, run, dist = (np.asarray(a, np.int64) for a in (lit, run, dist))
    is_ref = lit < 0
    ls = np.searchsorted(LEN_BASE, run[is_ref], side="right") - 1
    ds = np.searchsorted(DIST_BASE, dist[is_ref], side="right") - 1
    t = np.zeros((len(lit), 4), np.int64)
    t[:, 0], t[:, 2] = lit, -1
    t[is_ref, 0], t[is_ref, 1] = 257 + ls, run[is_ref] - LEN_BASE[ls]
    t[is_ref, 2], t[is_ref, 3] = ds, dist[is_ref] - DIST_BASE[ds]
    return t


def token_lengths(tokens, complete=True):
    """Huffman code lengths (literal/length: 286, distance: 30) for the histogram of these tokens and the end-of-block code;
    complete: a distance code of two codes at least, as zlib writes it -- otherwise one used distance symbol gets one code of one
    bit, and no used one leaves the lengths all 0"""
    tokens = np.asarray(tokens, np.int64).reshape(-1, 4)
    lhist = np.bincount(np.concatenate([tokens[:, 0], [256]]), minlength=286)
    dhist = np.bincount(tokens[tokens[:, 2] >= 0, 2], minlength=30)
    if complete and np.count_nonzero(dhist) < 2:
        dhist[:2] += 1
    dlen = huffman_lengths(dhist, 15) if np.count_nonzero(dhist) >= 2 else (dhist > 0).astype(np.int64)
    return huffman_lengths(lhist, 15), dlen


def header_items(seq, repeats=False):
    """the code lengths of a dynamic header (literal/length and distance lengths as ONE sequence, RFC 1951 3.2.7) as items
    (code-length symbol, extra bits' value, first index, lengths covered): one symbol per length, or -- repeats -- runs coded with
    16 / 17 / 18, which take no notice of where the literal/length lengths end"""
    seq = [int(v) for v in seq]
    if not repeats:
        return [(v, 0, i, 1) for i, v in enumerate(seq)]
    items, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        n, v = j - i, seq[i]
        if v == 0:
            while n >= 3:
                k = min(n, 138)
                items.append((18, k - 11, i, k) if k >= 11 else (17, k - 3, i, k))
                i, n = i + k, n - k
        else:
            items.append((v, 0, i, 1))
            i, n = i + 1, n - 1
            while n >= 3:
                k = min(n, 6)
                items.append((16, k - 3, i, k))
                i, n = i + k, n - k
        for _ in range(n):
            items.append((v, 0, i, 1))
            i += 1
    return items


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _token_fields(tokens, llen, dlen, eob):
    """the bit fields of the tokens of one block, and of its end-of-block code: four each (code, run's extra bits, distance code, its
    extra bits); literals leave three empty.  Length symbols 286 / 287 and distance symbols 30 / 31 have no extra bits; a distance
    symbol without a code takes no bits (a reference in a block that has no distance code)."""
    tokens = np.asarray(tokens, np.int64).reshape(-1, 4)
    lcode, dcode = canonical_codes(llen), canonical_codes(dlen)
    lx = np.zeros(288, np.int64); lx[257:286] = LEN_EXTRA
    dx = np.zeros(32, np.int64); dx[:30] = DIST_EXTRA
    n = len(tokens)
    sym, ref = tokens[:, 0], tokens[:, 2] >= 0
    assert np.all(llen[sym] > 0), "a token without a code"
    v = np.zeros((n + 1, 4), np.int64)
    b = np.zeros((n + 1, 4), np.int64)
    v[:n, 0], b[:n, 0] = lcode[sym], llen[sym]
    idx = np.nonzero(ref)[0]
    ds = tokens[idx, 2]
    assert np.all(tokens[idx, 1] < (1 << lx[sym[idx]])) and np.all(tokens[idx, 3] < (1 << dx[ds]))
    v[idx, 1], b[idx, 1] = tokens[idx, 1], lx[sym[idx]]
    v[idx, 2], b[idx, 2] = dcode[ds], dlen[ds]
    v[idx, 3], b[idx, 3] = tokens[idx, 3], np.where(dlen[ds] > 0, dx[ds], 0)
    if eob:
        v[n, 0], b[n, 0] = lcode[256], llen[256]
    return v.reshape(-1), b.reshape(-1)


def coded_block(llen, dlen, tokens, final=True, eob=True, repeats=False, nl=None, nd=None, clen=None):
    """ONE dynamic-Huffman block from explicit code lengths (llen: <= 288 of them, dlen: <= 32) and a token table -- rows (literal/
    length symbol, extra bits, distance symbol or -1, extra bits), symbols and extra bits as such -> (bytes, bits): raw DEFLATE, not
    padded beyond its last byte.  eob: the end-of-block code is written; repeats: the header's lengths are coded with 16 / 17 / 18;
    nl / nd: HLIT + 257 / HDIST + 1 (default: up to the last length that is not 0); clen: the code-length code's lengths
    (default: a Huffman code for the header's items).  Nothing is checked: that is the caller's business, or its intent."""
    ll = np.zeros(288, np.int64); ll[:len(llen)] = llen
    dl = np.zeros(32, np.int64); dl[:len(dlen)] = dlen
    if nl is None:
        nl = max(257, int(np.nonzero(ll)[0].max()) + 1)
    if nd is None:
        nd = max(1, int(np.nonzero(dl)[0].max()) + 1) if dl.any() else 1
    items = header_items(np.concatenate([ll[:nl], dl[:nd]]), repeats)
    isym = np.array([it[0] for it in items], np.int64)
    if clen is None:
        clen = huffman_lengths(np.bincount(isym, minlength=19), 7)
    clen = np.asarray(clen, np.int64)
    assert np.all(clen[isym] > 0)
    ccode = canonical_codes(clen)
    ncl = max(4, max(i for i, s in enumerate(CL_ORDER) if clen[s]) + 1)
    hv = [1 if final else 0, 2, nl - 257, nd - 1, ncl - 4] + [int(clen[s]) for s in CL_ORDER[:ncl]]
    hn = [1, 2, 5, 5, 4] + [3] * ncl
    for s, extra, _, _ in items:
        hv += [int(ccode[s]), extra]
        hn += [int(clen[s]), CL_EXTRA.get(s, 0)]
    v, b = _token_fields(tokens, ll, dl, eob)
    return pack_bits(np.concatenate([hv, v]), np.concatenate([hn, b]))


def fixed_block(tokens, final=True, eob=True):
    """ONE fixed-Huffman block of such a token table (RFC 1951, 3.2.6: 288 literal/length and 32 distance codes, the ones no
    valid stream uses included) -> (bytes, bits)"""
    ll = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, np.int64)
    v, b = _token_fields(tokens, ll, np.full(32, 5, np.int64), eob)
    return pack_bits(np.concatenate([[1 if final else 0, 1], v]), np.concatenate([[1, 2], b]))


def concat_bits(blocks):
    """(bytes, bits) pieces one behind the other at bit granularity -> (bytes, bits)"""
    bits = [np.unpackbits(np.frombuffer(by, np.uint8), bitorder="little")[:n] for by, n in blocks]
    allb = np.concatenate(bits) if bits else np.zeros(0, np.uint8)
    return np.packbits(allb, bitorder="little").tobytes(), len(allb)


def zlib_wrap(body, data):
    """raw DEFLATE and the bytes it inflates to -> a zlib stream"""
    return b"\x78\x01" + body + zlib.adler32(data).to_bytes(4, "big")


def gzip_wrap(body, data):
    """raw DEFLATE and the bytes it inflates to -> a gzip member without optional fields"""
    return (bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff]) + body + (zlib.crc32(data) & 0xffffffff).to_bytes(4, "little")
            + (len(data) & 0xffffffff).to_bytes(4, "little"))


def dynamic_block(lit, run, dist, final=True):
    """ONE dynamic-Huffman block of these tokens -> (bytes, bits): raw DEFLATE, not padded beyond its last byte (a Huffman code for
    their histogram, a complete distance code, the header's lengths one symbol each)"""
    tokens = symbol_tokens(lit, run, dist)
    llen, dlen = token_lengths(tokens)
    return coded_block(llen, dlen, tokens, final=final)


def one_dynamic_block(seed, out_bytes, **kw):
    """a zlib stream that is one final dynamic block -> (expected bytes, stream)"""
    body, _ = dynamic_block(*random_tokens(seed, out_bytes, **kw))
    data = zlib.decompressobj(-15).decompress(body)
    return data, zlib_wrap(body, data)


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
    vals = np.random.default_rng(seed + 1).integers(0, 144, n_fixed, dtype=np.uint8).astype(np.int64)
    z = np.zeros(n_fixed, np.int64)
    body, _ = concat_bits([dynamic_block(*random_tokens(seed, n_dynamic), final=False), fixed_block(symbol_tokens(vals, z, z))])
    data = zlib.decompressobj(-15).decompress(body)
    return data, zlib_wrap(body, data)
