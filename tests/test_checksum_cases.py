"""The checksum table (tests/checksum_cases.py) checked on the CPU: that its payloads are what they claim, that every mirror's peak is
the worst case the source names (or the shortfall, with the reason) and below 2^32, that the restated source lines are still there --
and the whole table through the emulators of tools/emu: inflate_kernel of csrc/inflate.hip, the pipeline of csrc/pinflate2.hip with one
workgroup and with 2, 3 and 7 parts, the search kernels of csrc/deflate.hip one-shot and pushed.  Each emulator twice: a plain build,
and one with -fsanitize=address,undefined (stand-alone programs, run as subprocesses, nothing preloaded), as tests/test_emu_bounds.py
builds them."""
import gzip
import os
import subprocess
import zlib

import pytest

import checksum_cases as cc
import geometry
import pnghelp as ph
from test_emu_bounds import SAN_ENV, sanitized
from test_emu_deflate import build as build_deflate
from test_emu_inflate import build_emu as build_inflate
from test_emu_pinflate import build_emu as build_pinflate
from test_oracle_gzip import gw

CSRC = ph.ROOT / "swift_png_amd" / "csrc"
LIMIT = 1 << 32


# ---- the table itself ----------------------------------------------------------------------------------------------------------------

def test_source_lines_are_still_there():
    text = {}
    for name, line in cc.SOURCE_LINES:
        if name not in text:
            text[name] = (CSRC / name).read_text()
        assert text[name].count(line) >= 1, (name, line)
    # each of the lines whose comparison a mirror relies on stands exactly where the mirror says: once in `flush`, twice in the inserters
    assert text["inflate.hip"].count("g = g >= 65521 ? g - 65521 : g;") == 1
    assert text["deflate.hip"].count("pm = pm + 64 >= 65521 ? pm + 64 - 65521 : pm + 64;") == 2
    assert text["deflate.hip"].count("accI += pm * byte;") == 2


def test_payloads_are_what_they_claim_and_stay_under_the_cap():
    assert len(set(cc.PAYLOADS)) == len(cc.PAYLOADS)
    assert sum(len(cc.payload(p)) for p in cc.PAYLOADS) <= cc.TOTAL_BYTES_CAP
    assert max(len(cc.payload(p)) for p in cc.ADLER_PAYLOADS) == cc.BASE_N == 262121
    assert cc.payload("high") == cc.payload("high") and min(cc.payload("high")) >= 0xF0 and len(set(cc.payload("high"))) == 16
    for p in cc.PAYLOADS:                                                        # the closed form itself, in unbounded integers
        d = cc.payload(p)
        assert cc.closed_form(*cc.adler_parts(d), len(d)) == zlib.adler32(d), p
    for n in cc.N_ZERO:
        assert len(cc.payload("n-zero-%d" % n)) == n
    assert sorted(n % cc.MOD for n in cc.N_ZERO) == [0, 0, 1, 65520]             # N = 0 (twice: one and two turns) and N = +-1
    assert zlib.adler32(cc.payload("s1-zero")) & 0xffff == 0 and sum(cc.payload("s1-zero")) == 65520
    assert zlib.adler32(cc.payload("s2-zero")) >> 16 == 0 and cc._s2_zero()[1] == cc.S2_ZERO_FOUND
    assert [cc.payload(t) for t in cc.TINY] == [b"", b"\xff", b"\xff\xff", b"\xff\xff\xff"]


def test_onehot_closed_forms():
    for p in cc.ONEHOT_P:
        d = cc.payload("onehot-%d" % p)
        assert d.count(0) == cc.BASE_N - 1 and d[p] == 0xFF
        assert cc.onehot_expected(p) == zlib.adler32(d), p
    assert {p % cc.MOD for p in cc.ONEHOT_P} >= {0, 1, 65519, 65520} and {p % 16 for p in cc.ONEHOT_P} >= {0, 15}


def test_gzip_piece_shapes():
    shapes = {n: cc.piece_shape(n) for n in cc.GZ_N}
    assert any(empty and not short for _, _, short, empty in shapes.values())     # empty trailing pieces behind full ones
    assert any(empty and short for _, _, short, empty in shapes.values())         # ... and behind a short one
    assert any(short and not empty for _, _, short, empty in shapes.values())     # a short last piece, the 256th
    assert any(full == cc.GZ_PIECES for _, full, _, _ in shapes.values())         # all pieces full
    lens = {ln for ln, _, _, _ in shapes.values()} | {cc.piece_len(cc.BASE_N)}
    assert cc.piece_len(cc.BASE_N) == cc.CRC_WAVE_THRESHOLD                       # the base length: pieces of exactly 1024 bytes, the last one shorter
    assert any(ln <= cc.CRC_WAVE_THRESHOLD for ln in lens) and any(ln > cc.CRC_WAVE_THRESHOLD for ln in lens)
    for n, (ln, full, short, empty) in shapes.items():
        assert full * ln + short == n and full + bool(short) + empty == cc.GZ_PIECES and short < ln


def test_peaks_of_flush_and_resolve():
    """inflate.hip `flush` names 65520*4080 + 30600 + 65520; pinflate2.hip names g * A < 2^29"""
    ff = cc.unit_peak(cc.payload("ff"))
    assert ff == cc.UNIT_WORST == 267352200          # 65520 = 16 * 4095: `ff` puts a whole unit of 0xFF on g = 65520
    assert cc.UNIT_WORST + 65520 < LIMIT and 65520 * 4080 < cc.UNIT_RESOLVE_CLAIM
    assert 65521 * 4080 + 30600 + 65520 < LIMIT      # (and with g one larger, should the conditional subtract ever let 65521 through)
    hi = cc.unit_peak(cc.payload("high"))
    assert 0xF0 * 16 * 65520 <= hi <= cc.UNIT_WORST  # `high`: at least sixteen 0xF0 on the same unit
    for p in cc.ADLER_PAYLOADS:
        assert cc.unit_peak(cc.payload(p)) + 65520 < LIMIT and cc.flush_accS_peak(cc.payload(p)) <= 65520 + 4 * 4080 and cc.tail_peak(cc.payload(p)) < LIMIT
    # the one-hots: the byte's position modulo 65521 times 255, plus its place in the unit
    for p in cc.ONEHOT_P:
        assert cc.unit_peak(cc.payload("onehot-%d" % p)) == 255 * ((p - p % 16) % cc.MOD) + 255 * (p % 16)
    # the bytes behind the last whole unit: BASE_N ends 9 bytes behind one; `ff` has 0xFF on all of them
    assert cc.BASE_N % 16 == 9 and cc.tail_peak(cc.payload("ff")) == 65520 + ((cc.BASE_N - 1) % cc.MOD) * 255


def test_peaks_of_the_search_inserter():
    """deflate.hip names "four products < 2^24 each on top of a reduced sum".  No payload reaches 4 * (2^24 - 1): the four batches of a
    quad are 64 positions apart for a lane, so at most one of them stands on 65520 -- the real worst case is INSERT_WORST, which `ff`
    reaches exactly (lane 48 of the quad at 65280), 0.65 % below the named bound."""
    assert 65520 * 255 < 1 << 24 and 65521 * 255 < 1 << 24
    assert cc.insert_peak(cc.payload("ff")) == cc.INSERT_WORST == 66732480 < cc.INSERT_CLAIM
    assert cc.INSERT_CLAIM + 65520 < LIMIT
    assert max(cc.insert_peak(cc.payload("ff"), warm) for warm in range(0, 65521, 4097)) <= cc.INSERT_WORST       # wherever a chunk begins
    for p in cc.ADLER_PAYLOADS:
        assert cc.insert_peak(cc.payload(p)) <= cc.INSERT_WORST
    # accS is reduced behind the chunk only: the longest chunk the launch arithmetic makes (one stream)
    chunks, positions = geometry.search_chunks(1)
    assert chunks >= 1 and cc.insert_accS_bound(positions) < LIMIT
    # the stored tail (n < 3)
    assert [cc.stored_tail_peak(cc.payload(t)) for t in cc.TINY[:3]] == [(0, 0), (255, 0), (510, 255)]


def test_peaks_of_the_resumed_adler():
    """gzip.hip resume_adler_kernel: I = (I + g * b) % 65521 and S += b over a lane's share of a piece"""
    peak_i, peak_s = cc.resume_peak(cc.payload("ff"))
    assert peak_i == cc.RESUME_WORST_I == 16707600 and peak_i + 65520 < LIMIT
    assert peak_s == 255 * (cc.piece_len(cc.BASE_N) // 64) == 4080                # 1024 bytes a piece: 16 bytes a lane
    # S: what the comment bounds.  A lane's S stays below 2^32 for pieces of up to RESUME_PIECE_LIMIT bytes -- 2^30 and more --, far
    # beyond the 2^24 a stream of 2^32 bytes has
    assert (cc.RESUME_PIECE_LIMIT // 64) * 255 < LIMIT and cc.RESUME_PIECE_LIMIT >= 1 << 30
    for p in cc.PAYLOADS:
        i, s = cc.resume_peak(cc.payload(p))
        assert i <= cc.RESUME_WORST_I and s <= 255 * -(-cc.piece_len(len(cc.payload(p))) // 64)


def test_streams_and_their_twins():
    for st in cc.all_streams():
        data = st.data
        if st.fmt == cc.ZLIB and st.status == cc.DONE:
            assert zlib.decompress(st.z) == data and st.z[-4:] == zlib.adler32(data).to_bytes(4, "big"), st.name
        if st.fmt == cc.RAW:
            assert zlib.decompress(st.z, -15) == data, st.name
        if st.fmt == cc.GZIP and st.status == cc.DONE:
            assert gzip.decompress(st.z) == data and st.z[-8:-4] == zlib.crc32(data).to_bytes(4, "little"), st.name
        if st.status != cc.DONE:
            twin = next(s for s in cc.streams(st.payload) if s.name == st.name[:-5])
            diff = [a ^ b for a, b in zip(st.z, twin.z) if a != b]
            assert len(diff) == 1 and bin(diff[0]).count("1") == 1 and st.aux[0] != st.aux[1], st.name
            assert st.aux[1] == (zlib.adler32(data) if st.fmt == cc.ZLIB else zlib.crc32(data))
    halves = {zlib.adler32(cc.payload(p)).to_bytes(4, "big")[k:k + 2] for p in ("s1-zero", "s2-zero") for k in (0, 2)}
    assert b"\0\0" in halves
    # the oracle's own Adler-32 agrees with Python's on every payload
    lib = ph.oracle()
    for p in cc.PAYLOADS:
        d = cc.payload(p)
        assert lib.orc_adler32(1, d, len(d)) == zlib.adler32(d), p


def test_gzip_expectation_is_the_wrapper_around_the_oracles_raw_stream():
    """cc.deflate_expected takes a gzip member's blocks from the oracle's zlib stream; at exponent 15 that is oracle/gzip_wrap.py's deflate
    over the oracle's raw format, byte for byte -- held here at every level for the payloads that cost the oracle little"""
    from test_oracle_gzip import raw_deflate
    for pname in ["ff", "n-zero-65521", "s1-zero", "s2-zero"] + cc.TINY + ["gz-257"]:
        for level in cc.DEFLATE_LEVELS:
            assert cc.deflate_expected(pname, level, cc.GZIP, 15) == gw.deflate(cc.payload(pname), raw_deflate(level)), (pname, level)
            assert gzip.decompress(cc.deflate_expected(pname, level, cc.GZIP, 8)) == cc.payload(pname)
    assert sorted(p for g in cc.DEFLATE_GROUPS.values() for p in g) == sorted(cc.ADLER_PAYLOADS)


# ---- the emulators -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu_inflate(tmp_path_factory):
    return build_inflate(tmp_path_factory.mktemp("emu_inflate_sums")), None


@pytest.fixture(scope="module")
def emu_inflate_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_inflate_sums_san")
    build_inflate(d)                                                             # (leaves the prepared sources in d)
    return sanitized(d, "emu_inflate.cpp", "EMU_INFLATE_SRC", d / "inflate_emu.inc"), SAN_ENV


@pytest.fixture(scope="module")
def emu_pinflate(tmp_path_factory):
    return build_pinflate(tmp_path_factory.mktemp("emu_pinflate_sums") / "emu_pinflate2"), None


@pytest.fixture(scope="module")
def emu_pinflate_san(tmp_path_factory):
    # (-fno-sanitize=bounds: tests/test_emu_bounds.py says why)
    return sanitized(tmp_path_factory.mktemp("emu_pinflate_sums_san"), "emu_pinflate2.cpp", defines=("-fno-sanitize=bounds",)), SAN_ENV


@pytest.fixture(scope="module")
def emu_deflate(tmp_path_factory):
    return build_deflate(tmp_path_factory.mktemp("emu_deflate_sums")), None


@pytest.fixture(scope="module")
def emu_deflate_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_deflate_sums_san")
    build_deflate(d)
    return sanitized(d, "emu_deflate2.cpp", "EMU_DEFLATE_SRC", d / "deflate_emu.inc", ("-DSPNG_D3_WAVES=4",)), SAN_ENV


# The sanitized builds switch fibers through ucontext and are slow where a stream has many tokens: `high` at 262121 bytes takes 184 s in
# emu_inflate and 40 s in emu_pinflate2, a stream of under 300 bytes that inflates to 262121 about 9 s.  What they add to the plain
# builds is the address and undefined-behaviour checks, not arithmetic (unsigned overflow is defined).  So they take every stream of
# the payloads of up to 600 bytes and of the one of 4097 (SMALL) and, of the payloads that drive a sum to its limit, the zlib-made zlib
# stream: `ff`, every one-hot, and `n-zero-65521` for `high`'s kind (SAN_LARGE).  Left to the plain builds alone: `high` and
# `gz-262145` (minutes each), the other three n-zero lengths and gz-65535 / gz-65537 (about a minute each in emu_inflate), gz-4095 / gz-4096.
SMALL = [p for p in cc.PAYLOADS if len(cc.payload(p)) <= 600 or p == "gz-4097"]
SAN_LARGE = ["ff"] + cc.ONEHOTS + ["n-zero-65521"]


def chosen(pname, only):
    """the streams of a payload; only: the one the sanitized builds take of a large payload"""
    return [st for st in cc.streams(pname) if not only or st.name == pname + "/zlib6/zlib"]


@pytest.mark.parametrize("pname", cc.PAYLOADS)
def test_serial_kernel_over_the_table(emu_inflate, tmp_path, pname):
    """`flush`: every stream of the payload; a twin answers SPNG_E_STREAM_CHECKSUM with (declared, the right sum).  A gzip member goes in
    as the kernel sees it: the raw payload, the trailer behind it (the CRC-32 is gzip.hip's: tests/test_emu_gzip.py)"""
    serial(emu_inflate, tmp_path, pname)


@pytest.mark.parametrize("pname", SMALL + SAN_LARGE)
def test_serial_kernel_under_the_sanitizers(emu_inflate_san, tmp_path, pname):
    serial(emu_inflate_san, tmp_path, pname, only=pname in SAN_LARGE)


def serial(emu_inflate, tmp_path, pname, only=False):
    exe, env = emu_inflate
    for st in chosen(pname, only):
        if st.fmt == cc.GZIP and st.status != cc.DONE:
            continue
        z, fmt = cc.body(st)
        (tmp_path / "z").write_bytes(z)
        r = subprocess.run([str(exe), str(tmp_path / "z"), str(fmt), str(len(st.data)), str(tmp_path / "out")], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, (st.name, r.returncode, r.stdout[-300:], r.stderr[-3000:])
        status, written, consumed, aux0, aux1 = (int(x) for x in r.stdout.split())
        assert (status, written) == (st.status, len(st.data)) and (tmp_path / "out").read_bytes() == st.data, (st.name, r.stdout)
        if st.status == cc.DONE:
            assert consumed == len(z) - (8 if st.fmt == cc.GZIP else 0), (st.name, r.stdout)
        else:
            assert (aux0, aux1) == st.aux, (st.name, r.stdout, st.aux)


def pipeline(emu_pinflate, tmp_path, st, parts):
    """-> (the run, the number of parts the plan made)"""
    exe, env = emu_pinflate
    (tmp_path / "z").write_bytes(st.z)
    (tmp_path / "raw").write_bytes(st.data)
    e = dict(os.environ if env is None else env, **({"EMU_PARTS": str(parts)} if parts else {}))
    r = subprocess.run([str(exe), str(tmp_path / "z"), str(tmp_path / "raw"), str(st.fmt), "256"], capture_output=True, text=True, timeout=900, env=e)
    ran = [int(line.split()[1]) for line in r.stdout.splitlines() if line.startswith("parts:")]
    return r, (ran[0] if ran else 1)


@pytest.mark.parametrize("pname", [p for p in cc.PAYLOADS if p != "tiny-0"])
def test_pipeline_over_the_table_with_one_workgroup_and_in_parts(emu_pinflate, tmp_path, pname):
    resolve(emu_pinflate, tmp_path, pname)


@pytest.mark.parametrize("pname", [p for p in SMALL if p != "tiny-0"] + SAN_LARGE)
def test_pipeline_under_the_sanitizers(emu_pinflate_san, tmp_path, pname):
    resolve(emu_pinflate_san, tmp_path, pname, only=pname in SAN_LARGE)


def test_pipeline_resolves_in_exactly_the_parts_asked_for(emu_pinflate, tmp_path):
    """2, 3 and 7 parts, each honoured in full, on the payload long enough for seven (cc.PARTS7): zlib's stream, the oracle's, its raw
    form, and their twins.  tests/test_gpu_checksum_cases.py runs the same streams and reads the same count from the device."""
    for st in cc.streams(cc.PARTS7):
        if st.fmt == cc.GZIP:
            continue
        for parts in (2, 3, 7):
            r, ran = pipeline(emu_pinflate, tmp_path, st, parts)
            answered(r, st, parts)
            assert ran == parts, (st.name, parts, ran)


def answered(r, st, parts):
    if st.status == cc.DONE:
        assert r.returncode == 0 and "ok:" in r.stdout, (st.name, parts, r.returncode, r.stdout[-300:], r.stderr[-3000:])
    else:
        assert r.returncode == 5 and ("error %d aux %x %x written %d " % (st.status, st.aux[0], st.aux[1], len(st.data))) in r.stdout, (
            st.name, parts, r.returncode, r.stdout[-300:], r.stderr[-3000:])


def resolve(emu_pinflate, tmp_path, pname, only=False):
    """the tile loop, the bytes behind the last unit, and -- with 2, 3 and 7 parts forced -- pinf2_fixup_kernel and pinf2_verdict_kernel.
    Segments of 256 bytes.  A part begins at a segment that starts a block behind the first 32 KiB, so the plan makes fewer parts than
    asked where a stream has few blocks: what it made is read from the driver, and the streams that must split (cc.splits) are held to
    two parts or more; 262121 bytes are too few for seven (the test above has the payload that is long enough).  One workgroup: every
    stream; in parts: the zlib stream and its twin of either encoder -- the raw form drives the same sums."""
    for st in chosen(pname, only):
        if st.fmt == cc.GZIP:
            continue                                                             # (the same kernels as the raw stream: gzip.hip moves the window)
        for parts in (0, 2, 3, 7) if st.fmt == cc.ZLIB else (0,):
            r, ran = pipeline(emu_pinflate, tmp_path, st, parts)
            answered(r, st, parts)
            if parts and cc.splits(st):
                assert 2 <= ran <= parts, (st.name, parts, ran)                  # markers, windows, the fold over parts
            if parts == 0:
                assert ran == 1


def deflate_run(emu_deflate, tmp_path, pname, level, cuts=(), **knobs):
    exe, env = emu_deflate
    data = cc.payload(pname)
    want = ph.orc_deflate(data, level, cc.ZLIB)
    assert want[-4:] == zlib.adler32(data).to_bytes(4, "big") and zlib.decompress(want) == data
    (tmp_path / "in").write_bytes(data)
    (tmp_path / "want").write_bytes(want)
    r = subprocess.run([str(exe), str(tmp_path / "in"), str(tmp_path / "want"), str(level), "0", "2"] + [str(c) for c in cuts], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ if env is None else env, **knobs))
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (pname, level, cuts, knobs, r.returncode, r.stdout[-300:], r.stderr[-3000:])


EMU_LEVELS = (0, 1, 6, 8, 13)
CUTS = (65520, 65521, 65522)


@pytest.mark.parametrize("pname", cc.ADLER_PAYLOADS)
def test_search_kernels_over_the_table(emu_deflate, tmp_path, pname):
    search(emu_deflate, tmp_path, pname, EMU_LEVELS)


# emu_deflate2 under the sanitizers costs about 95 s for a payload of 262121 bytes (levels 1 and 8, one-shot and a push each), so of the
# one-hots it takes the two on either side of the modulus.  `n-zero-65521` keeps to level 1: in the full search of noise the address
# sanitizer stops at d2_forward's blind read of the word behind g_ptab, an LDS value nobody uses, as tests/test_emu_bounds.py found for
# its 70 000-byte input at level 9 (profiles/r17_bounds.md has the report).
SAN_LARGE_DEFLATE = {"ff": (1, 8), "onehot-65520": (1, 8), "onehot-65521": (1, 8), "n-zero-65521": (1,)}


@pytest.mark.parametrize("pname", [p for p in SMALL if p in cc.ADLER_PAYLOADS] + list(SAN_LARGE_DEFLATE))
def test_search_kernels_under_the_sanitizers(emu_deflate_san, tmp_path, pname):
    """(the large payloads at one level per search kernel: the sums are the inserter's, the same at every level)"""
    search(emu_deflate_san, tmp_path, pname, SAN_LARGE_DEFLATE.get(pname, EMU_LEVELS))


def search(emu_deflate, tmp_path, pname, levels):
    """d3_insert_quad (and d3_insert for a chunk's ragged last quad) in both search kernels, adler32_word, the stored tail: the stream,
    trailer included, is the oracle's byte for byte.  One-shot, and -- where the payload is that long -- pushed in three pieces: all
    three first cuts at levels 1 and 8 (one per search kernel), one of them, a different one per level, at the others."""
    for level in levels:
        deflate_run(emu_deflate, tmp_path, pname, level)
    n = len(cc.payload(pname))
    if n > CUTS[-1]:
        for k, level in enumerate(levels):
            for cut in CUTS if level in (1, 8) and len(levels) > 2 else CUTS[k % 3:k % 3 + 1]:
                deflate_run(emu_deflate, tmp_path, pname, level, cuts=(cut, cut + 70001) if cut + 70001 < n else (cut,))


@pytest.mark.parametrize("pname", ["ff", "onehot-65520", "n-zero-65521"])
def test_search_kernels_with_the_read_back_inserter(emu_deflate, tmp_path, pname):
    """The emulator takes the exchange form of the inserter, as the device does where its LDS serves a bucket's lanes in order: there
    d3_insert sums only a chunk's ragged last quad.  EMU_D3_READBACK = 1 takes the other form, in which d3_insert sums every position."""
    for level in (1, 8):
        deflate_run(emu_deflate, tmp_path, pname, level, EMU_D3_READBACK="1")
