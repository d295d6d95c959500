"""The tables of tests/bounds_cases.py held to their claims, on the CPU: every named capacity lies where its name says (read from
the stream's tokens), the oracle answers as the tables assume, no capacity stands twice in a stream's rows, and every deflate stream
fits the product's bound."""
import zlib

import pytest

import bounds_cases as bc
import deflate_tokens as dt
import pnghelp as ph


def term_at(blks, pos):
    """-> (block, term) that holds output byte `pos`"""
    for b in blks:
        for t in b.terms:
            if t[0] <= pos < t[0] + (t[1] if len(t) == 3 else 1):
                return b, t
    raise AssertionError(pos)


@pytest.mark.parametrize("name", bc.STREAMS)
def test_inflate_streams_are_what_they_claim(name):
    st, blks = bc.stream(name), bc.blocks(name)
    assert dt.length(blks) == st.n
    assert zlib.decompressobj(-15).decompress(st.z[st.body_at:st.body_at + st.body_len]) == st.data
    kinds = [b.kind for b in blks]
    if name in ("a", "a-raw", "a-gzip"):
        assert st.n == 49152 and kinds.count("dynamic") >= 2
    if name == "b":
        assert sum(1 for b in blks if b.kind == "stored" and not b.count) >= 5           # (the flushes' empty stored blocks)
    if name == "c":
        assert st.n == 30000 and set(kinds) == {"stored"}
    if name == "periods":
        assert len(blks) == 1 and st.n > 3_000_000
    if name == "a-gzip":
        assert st.z[3] == 0x0c and st.body_at == 10 + 2 + 7 + 9                          # FEXTRA | FNAME


@pytest.mark.parametrize("name", bc.STREAMS)
def test_inflate_capacities_lie_where_their_names_say(name):
    st, blks, rows = bc.stream(name), bc.blocks(name), dict(bc.inflate_rows(name))
    N = st.n
    assert len(rows) == len(bc.inflate_rows(name)) and len(set(rows.values())) == len(rows)      # no name and no capacity twice
    for k, v in (("N", N), ("N+1", N + 1), ("N-1", N - 1), ("N-15", N - 15), ("N-16", N - 16), ("N-17", N - 17), ("0", 0), ("1", 1),
                 ("15", 15), ("16", 16), ("17", 17)):
        assert rows[k] == v
    assert ("32768" in rows) == ("32769" in rows) == (N > 32769)
    stored_only = all(b.kind == "stored" for b in blks)
    assert ("inside-match" in rows) == ("match-end" in rows) == (not stored_only)
    if "inside-match" in rows:
        cap = rows["inside-match"]
        _, t = term_at(blks, cap)
        assert len(t) == 3 and t[0] < cap < t[0] + t[1]                                  # strictly inside: bytes of it on both sides
        # (zlib finds no match of 64 bytes in the scanline generator's output; there the row lies in the stream's longest match)
        assert t[1] >= (64 if name in ("periods", "echo") else 3)
        if name == "periods":
            assert t[1] == 258
        _, t = term_at(blks, rows["match-end"] - 1)
        assert len(t) == 3 and t[0] + t[1] == rows["match-end"]
    assert "block-boundary" in rows or len(blks) == 1
    if "block-boundary" in rows:
        cap = rows["block-boundary"]
        assert any(b.terms and b.terms[0][0] == cap for b in blks[1:]) and 0 < cap < N
    assert ("inside-stored" in rows) == (name == "c")
    if name == "c":
        cap = rows["inside-stored"]
        b, _ = term_at(blks, cap)
        assert b.kind == "stored" and b.terms[0][0] < cap < b.terms[-1][0]
    assert ("at-empty-stored" in rows) == (name == "b")
    if name == "b":
        cap = rows["at-empty-stored"]
        assert any(b.kind == "stored" and not b.count and bc._position(blks, k) == cap for k, b in enumerate(blks))
    assert ("inside-literals" in rows) == (name != "c")
    if "inside-literals" in rows:
        cap = rows["inside-literals"]
        (b0, t0), (b1, t1) = term_at(blks, cap - 1), term_at(blks, cap)
        assert b0 is b1 and b0.kind != "stored" and len(t0) == len(t1) == 2


@pytest.mark.parametrize("name", bc.STREAMS)
def test_oracle_answers_every_inflate_row_as_the_table_assumes(name):
    st = bc.stream(name)
    for label, cap in bc.inflate_rows(name):
        status, out, consumed, aux = bc.inflate_expected(name, cap)
        if cap >= st.n:
            assert (status, out, consumed) == (0, st.data, len(st.z)), (name, label)
        else:
            assert status == bc.E_OUTPUT_CAPACITY and len(out) <= cap and out == st.data[:len(out)], (name, label, status, len(out))


@pytest.mark.parametrize("level", bc.LEVELS)
def test_deflate_rows(level):
    bound = ph.oracle().orc_deflate_bound
    dropped_of = {}
    for name, lv, fmt, e in bc.deflate_streams(level):
        data, f = bc.inputs()[name], bc.full(name, lv, fmt, e)
        n, L = len(data), len(f)
        assert L <= n + n // 4 + 4096 and L <= bound(n) + (18 if fmt == bc.GZIP else 0)  # spng_deflate_bound; the oracle's own
        # the oracle's stream is a stream: header, body, trailer
        if fmt == bc.ZLIB:
            assert f[0] == (e - 8) << 4 | 8 and zlib.decompress(f, wbits=15) == data and f[-4:] == zlib.adler32(data).to_bytes(4, "big")
        elif fmt == bc.RAW:
            assert zlib.decompressobj(-15).decompress(f) == data
        else:
            assert f[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff]) and f[10:-8] == bc.full(name, lv, bc.RAW)
            assert f[-8:] == zlib.crc32(data).to_bytes(4, "little") + (n & 0xffffffff).to_bytes(4, "little")
        kept, dropped = bc.deflate_caps(L)
        rows = dict(kept)
        dropped_of.setdefault(name, set()).update(dropped)
        # the named positions are what they claim for this L
        assert rows["L"] == L and rows["L+1"] == L + 1 and rows["L//2|1"] % 2 == 1
        if fmt == bc.ZLIB and "L-5" in rows:
            assert L - 4 <= rows["L-4"] < L and rows["L-5"] < L - 4                      # inside, and in front of, the Adler-32
        if fmt == bc.GZIP:
            assert L >= 18 and rows["L-8"] == L - 8 and L - 8 <= rows["L-4"] < L and rows["L-9"] == L - 9 >= 10 - 1
            assert rows["9"] < 10 <= rows["10"] and rows["10"] == 10                     # inside, and behind, the ten header bytes
        for c in bc.SOMETIMES:
            assert (c in rows) == (int(c) < L)
        if "1024" in rows:
            assert rows["1023"] < bc.OUTB // 2 == rows["1024"] < rows["1025"] and rows["2049"] == bc.OUTB + 1
        for label, cap in kept:
            status, written, consumed, head = bc.deflate_expected(name, lv, fmt, e, cap)
            assert (status == 0) == (cap >= L) and written == L and consumed == n and head == f[:min(cap, L)]
    # rows that L is too short for: the four around the ring (1023 ... 2049), and L - 5, L - 8, L - 9 where they are negative, which
    # only the inputs of 0 ... 4 bytes in the raw format (L = 5 ... 8) see
    for name, dropped in dropped_of.items():
        n = len(bc.inputs()[name])
        assert len(dropped) <= (4 if n >= 200 else 7), (name, dropped)
        if n >= 5000:
            assert not dropped, (name, dropped)
