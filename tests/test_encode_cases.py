"""The encoder's case table (tests/encode_cases.py) without a GPU: every (case, level) is PROVEN from the oracle's own tokens -- the
stream orc_deflate writes, read back by the plain reader of tests/deflate_tokens.py, holds exactly the planted matches and
literals otherwise -- and then the device's kernels, run by the wave emulator as tests/test_emu_deflate.py builds it, must write
the same bytes under every knob the emulator has: chunk geometry, the read-back inserter, the two-wave parse, input in pieces,
rounds of 2^14 positions."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_tokens as dt
import encode_cases as ec
import pnghelp as ph
from test_emu_deflate import build


# ---- the reader ----------------------------------------------------------------------------------------------------------------

def _rebuild(blocks):
    out = bytearray()
    for blk in blocks:
        for t in blk.terms:
            assert t[0] == len(out)
            if len(t) == 2:
                out.append(t[1])
            else:
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def _reader_inputs():
    rng = np.random.default_rng(3)
    return {"empty": b"", "one": b"x", "text": b"to be or not to be, that is the question; " * 40, "zeros": bytes(70000),
            "noise": rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), "few": rng.integers(0, 3, 20000, dtype=np.uint8).tobytes()}


@pytest.mark.parametrize("kind", sorted(_reader_inputs()))
def test_reader_agrees_with_zlib(kind):
    """stored, fixed and dynamic blocks, zlib and raw: the tokens rebuild what zlib.decompress gives, blocks tile the stream's bits"""
    data = _reader_inputs()[kind]
    for level, strategy, wbits in ((0, zlib.Z_DEFAULT_STRATEGY, 15), (6, zlib.Z_FIXED, 15), (9, zlib.Z_DEFAULT_STRATEGY, 15), (1, zlib.Z_DEFAULT_STRATEGY, -15),
                                   (6, zlib.Z_HUFFMAN_ONLY, 9)):
        co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
        z = co.compress(data) + co.flush()
        blocks = dt.read(z, raw=wbits < 0)
        assert _rebuild(blocks) == zlib.decompressobj(wbits).decompress(z) == data
        assert dt.length(blocks) == len(data)
        assert blocks[-1].final and not any(b.final for b in blocks[:-1])
        assert blocks[0].first_bit == (0 if wbits < 0 else 16)
        for a, b in zip(blocks, blocks[1:]):
            assert a.last_bit < b.first_bit <= a.last_bit + 8 and (a.kind == "stored" or b.kind == "stored" or b.first_bit == a.last_bit + 1)
        kinds = {b.kind for b in blocks}
        assert kinds == {"stored"} if level == 0 else "dynamic" not in kinds if strategy == zlib.Z_FIXED else True      # (zlib stores what does not shrink)


def _fixed_block(symbols):
    """a final fixed-code block from (value, bits, huffman) fields: Huffman codes go MSB first, everything else LSB first"""
    acc = n = 0
    for value, bits, huffman in [(1, 1, False), (1, 2, False)] + symbols:
        if huffman:
            value = int(format(value, "0%db" % bits)[::-1], 2)
        acc |= value << n
        n += bits
    return acc.to_bytes((n + 7) // 8, "little")


def test_reader_raises_on_malformed_streams():
    z = zlib.compress(b"to be or not to be, that is the question; " * 40, 9)
    raw = z[2:-4]
    assert dt.read(raw, raw=True) and dt.read(z)
    a, end, run3, dist2 = (0x30 + 97, 8, True), (0, 7, True), (1, 7, True), (1, 5, True)
    assert dt.matches(dt.read(_fixed_block([a, a, run3, dist2, end]), raw=True)) == [(2, 3, 2)]
    bad = {
        "truncated": (raw[:-3], True), "bytes behind the end": (raw + b"\0", True), "reserved block type": (bytes([raw[0] | 6]) + raw[1:], True),
        "zlib method": (bytes([z[0] ^ 1]) + z[1:], False), "zlib check bits": (z[:1] + bytes([z[1] ^ 1]) + z[2:], False), "zlib trailer": (z[:-1], False),
        "stored LEN / NLEN": (b"\x01\x03\x00\xfc\xfe" + b"abc", True),
        "distance in front of the output": (_fixed_block([a, run3, dist2, end]), True),
        "length symbol 286": (_fixed_block([a, (0xc6, 8, True), dist2, end]), True),
        "distance symbol 30": (_fixed_block([a, a, run3, (30, 5, True), end]), True),
        "HLIT 287": (bytes([0x05 | (30 << 3) & 0xff]) + bytes(20), True),
        "no end of block": (_fixed_block([a, a]), True),
    }
    for what, (s, is_raw) in bad.items():
        with pytest.raises(dt.Malformed):
            dt.read(s, raw=is_raw)


# ---- the table -----------------------------------------------------------------------------------------------------------------

def test_every_case_states_what_it_expects():
    assert len(set(ec.NAMES)) == len(ec.NAMES) > 90
    for name in ec.NAMES:
        c = ec.case(name)
        assert c.levels and c.purpose and len(c.purpose) > 20, name
        assert c.exponent in range(8, 16)
        for lv in c.levels:
            assert lv in c.expect and isinstance(c.expect[lv], list), (name, lv)
            assert c.expect[lv] or c.empty, (name, lv, "a case without a planted match says so")
            assert c.expect[lv] == sorted(c.expect[lv]) and all(5 < r <= 258 and 0 < d <= a and d < 1 << c.exponent for a, r, d in c.expect[lv]), (name, lv)
        assert any(c.expect[lv] for lv in c.levels) or c.empty
        assert len(c.data) <= 160_000 or name.startswith(("round-edge-", "dense-block")), (name, len(c.data))
    for family in ("edge-e8-", "edge-e11-", "edge-e15-", "second-e8-", "second-e11-", "second-e15-", "bucket-foreign", "bucket-same-batch", "attempts-", "goal-", "equal-", "lazy-tie",
                   "lazy-win", "lazy-chain", "tail-run-", "tail-end-", "tail-cut-", "tail-tiny-", "far-gap-", "far-sweep-", "chunk-edge-32768-", "chunk-edge-65536-",
                   "chunk-edge-40384-", "block-edge-", "dense-block", "round-edge-"):
        assert any(n.startswith(family) for n in ec.NAMES), family
    # both sides of every attempts / goal value of the level table
    for lv in ec.ALL:
        assert {f"attempts-{ec.ATTEMPTS[lv] - 1}", f"attempts-{ec.ATTEMPTS[lv]}", f"goal-{ec.GOAL[lv] - 1}", f"goal-{ec.GOAL[lv]}"} <= set(ec.NAMES)


def _prove(c):
    for lv in c.levels:
        z = ph.orc_deflate(c.data, lv, 0, c.exponent)
        assert zlib.decompress(z) == c.data, (c.name, lv)
        assert z[0] >> 4 == c.exponent - 8
        blocks = dt.read(z)
        assert dt.length(blocks) == len(c.data), (c.name, lv)
        got = dt.matches(blocks)
        assert got == c.expect[lv], (c.name, lv, c.purpose, [t for t in got if t not in c.expect[lv]][:5], [t for t in c.expect[lv] if t not in got][:5])
        for k, count in c.blocks.get(lv, {}).items():
            assert blocks[k].count == count, (c.name, lv, c.purpose, k, [b.count for b in blocks][:20])


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_is_proven_by_the_oracles_tokens(name):
    _prove(ec.case(name))


def test_block_cases_name_every_block_they_speak_of():
    for name in ec.NAMES:
        if name.startswith(("block-edge-", "dense-block")):
            c = ec.case(name)
            for lv in c.levels:
                assert len(c.blocks[lv]) >= (3 if name == "dense-block" else 2), (name, lv)


# ---- the emulator --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build(tmp_path_factory.mktemp("emu_encode"))


@pytest.fixture(scope="module")
def emu_small_rounds(tmp_path_factory):
    return build(tmp_path_factory.mktemp("emu_encode_rv"), 1 << 14)


class Runner:
    """a case's input and the oracle's streams on disk once; run(exe, level, chunks, cuts, **env)"""

    def __init__(self, tmp_path, c):
        self.c, self.dir = c, tmp_path
        (tmp_path / "in").write_bytes(c.data)
        self.want = {}

    def run(self, exe, lv, chunks, cuts=(), **env):
        c = self.c
        if lv not in self.want:
            self.want[lv] = self.dir / f"want{lv}"
            self.want[lv].write_bytes(ph.orc_deflate(c.data, lv, 0, c.exponent))
        r = subprocess.run([str(exe), str(self.dir / "in"), str(self.want[lv]), str(lv), "0", str(chunks)] + [str(x) for x in cuts], capture_output=True, text=True,
                           timeout=900, env=dict(os.environ, EMU_EXPONENT=str(c.exponent), **env))
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (c.name, lv, chunks, cuts, env, c.purpose, r.stdout[-300:], r.stderr[-300:])
        return r.stdout


# One chunk for the whole stream (the ring wraps), and the product's two geometries for streams below 2 MiB: 64 chunks per round
# = chunks of 32768 positions (a stream alone), 52 = chunks of 40384 (five streams).  With the product's rounds of 2^21 positions
# 2 or 5 chunks per round start at 2^20 and 419456, behind every case's end, so those run on the build with rounds of 2^14 positions:
# chunks of 16384, 8192 and 3328 positions, which fall on, in front of and behind the planted places.
CHUNKS, SMALL_CHUNKS = (1, 64, 52), (1, 2, 5)


@pytest.mark.parametrize("name", [n for n in ec.NAMES if not n.startswith("round-edge-")])
def test_emulated_kernels_write_the_oracles_stream(emu, emu_small_rounds, tmp_path, name):
    c = ec.case(name)
    run = Runner(tmp_path, c)
    for lv in c.levels:
        for chunks in CHUNKS:
            assert "blocks side by side" in run.run(emu, lv, chunks)
        for chunks in SMALL_CHUNKS:
            run.run(emu_small_rounds, lv, chunks)
        if name.startswith(("bucket-", "second-")):
            run.run(emu, lv, 64, EMU_D3_READBACK="1")
            run.run(emu_small_rounds, lv, 5, EMU_D3_READBACK="1")
        if name.startswith(("block-edge-", "lazy-")):
            assert "blocks side by side" not in run.run(emu, lv, 64, EMU_TWO_WAVE="1")
            run.run(emu_small_rounds, lv, 2, EMU_TWO_WAVE="1")
        if name.startswith(("lazy-", "tail-", "block-edge-")):
            cuts = ec.cuts(c, lv)
            if cuts:
                run.run(emu, lv, 64, cuts)
                run.run(emu_small_rounds, lv, 2, cuts)
                if lv in (c.levels[0], c.levels[-1]):          # ... and each cut alone, two pushes: a greedy level and a lazy one
                    for cut in cuts:
                        run.run(emu, lv, 64, (cut,))


@pytest.mark.parametrize("variant", ec.ROUND_VARIANTS)
def test_round_boundary_plants(emu_small_rounds, tmp_path, variant):
    """rounds of 2^14 positions: a lazy pair over a round's last position and the one behind it, a run across the boundary, a
    run at the next round's first position with its source 32767 back -- proven from tokens, then emulated, one-shot and in pieces"""
    c = ec.round_small(variant)
    _prove(c)
    run = Runner(tmp_path, c)
    for lv in c.levels:
        for chunks in SMALL_CHUNKS:
            out = run.run(emu_small_rounds, lv, chunks)
            assert int(out.split(" in ")[1].split()[0]) == 4, out
        run.run(emu_small_rounds, lv, 2, EMU_TWO_WAVE="1")
        run.run(emu_small_rounds, lv, 2, ec.cuts(c, lv))


@pytest.mark.parametrize("variant", ec.ROUND_VARIANTS)
def test_round_boundary_twin_at_full_size(emu, tmp_path, variant):
    """the twin for the device, plants around position 2^21: two rounds of the product's size on the emulator"""
    c = ec.case(f"round-edge-{variant}")
    run = Runner(tmp_path, c)
    for lv in c.levels:
        assert " in 2 rounds" in run.run(emu, lv, 64)
