"""Block cuts for a resumed call (csrc/pinflate2.hip: "resumed calls" -- the anchor that starts at a token, the hand-over of the tail
to the serial kernel) on the CPU, by the wave emulator of tools/emu, driven as tests/test_emu_blockcuts.py drives it.  The input is a
one-block stream cut short -- in a resumed call the input usually ends inside the block --, the state stands inside the block, and
the first bytes of the output are there, as an earlier call would have left them."""
import os
import re
import shutil
import subprocess

import pytest

import oneblock as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 2048


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("emu") / "emu_pinflate2"
    subprocess.run(["g++", "-O1", "-std=c++17", "-DSPNG_EMU", "-I" + os.path.join(ROOT, "tools", "emu"), "-x", "c++", "-fpermissive",
                    "-Wno-attributes", "-w", "-o", str(out), os.path.join(ROOT, "tools", "emu", "emu_pinflate2.cpp")],
                   check=True, capture_output=True, timeout=600)
    return out


def run(emu, tmp, z, data, state, cut=8192):
    """the emulator over the stream so far with the state {header bit, bytes in front of the block, token bit, bytes written}
    -> (exit code, (tried, joined, redone) or None, (bit, bytes, header bit, header bytes) of the hand-over or None, log)"""
    (tmp / "z").write_bytes(z)
    (tmp / "want").write_bytes(data)
    env = dict(os.environ)
    for k in ("EMU_CUT_BYTES", "EMU_PARTS", "EMU_VERBOSE", "EMU_TOK_BIT", "EMU_TOK_OUT"):
        env.pop(k, None)
    if cut:
        env.update(EMU_CUT_BYTES=str(cut), EMU_TOK_BIT=str(state[2]), EMU_TOK_OUT=str(state[3]))
    r = subprocess.run([str(emu), str(tmp / "z"), str(tmp / "want"), "0", str(SEG), "4096", str(state[0]), str(state[1])],
                       capture_output=True, text=True, timeout=900, env=env)
    m = re.search(r"cuts tried=(\d+) joined=(\d+) redone=(\d+)", r.stdout)
    h = re.search(r"handover bit=(\d+) bytes=(\d+) header=(\d+) header_bytes=(\d+)", r.stdout)
    return (r.returncode, tuple(int(g) for g in m.groups()) if m else None, tuple(int(g) for g in h.groups()) if h else None,
            r.stdout + r.stderr)


@pytest.mark.parametrize("k", [5000, 100000])
def test_fixed_block_resumed_at_a_token(emu, tmp_path, k):
    """literals of eight bits behind a three-bit header at bit 16: token k starts at bit 19 + 8 k with k bytes written"""
    data, z = ob.one_fixed_block(2, 200000)
    z = z[:len(z) * 3 // 4]
    rc, stats, hand, log = run(emu, tmp_path, z, data, (16, 0, 19 + 8 * k, k))
    assert rc == 0 and "MISMATCH" not in log, log                # (every byte up to the hand-over equals zlib's)
    tried, joined, redone = stats
    assert tried >= 8 and joined >= 1 and redone == 0, log
    assert hand is not None, log
    b, nbytes, hdr, hdr_bytes = hand
    assert (hdr, hdr_bytes) == (16, 0)
    assert (b - 19) % 8 == 0 and nbytes == (b - 19) // 8, hand
    assert nbytes > k and 0 <= len(z) * 8 - b <= 2 * SEG * 8, (hand, len(z))


def test_a_short_rest_is_left_alone(emu, tmp_path):
    """less than the threshold behind the token: no cut is tried, the call goes the way it went before"""
    data, z = ob.one_fixed_block(2, 200000)
    z = z[:len(z) * 3 // 4]
    k = len(z) - 4096
    rc, stats, hand, log = run(emu, tmp_path, z, data, (16, 0, 19 + 8 * k, k))
    assert rc == 0 and stats is None and hand is None, log


def token_starts(body):
    """a plain bit-walk over ONE dynamic block (RFC 1951, 3.2.7) that starts at bit 0 of body: -> {bit a token starts at: bytes
    in front of it}, up to the end-of-block code or the end of the input"""
    n = len(body) * 8

    def bits(at, k):                                              # (k <= 13)
        return (int.from_bytes(body[at >> 3:(at >> 3) + 4], "little") >> (at & 7)) & ((1 << k) - 1)

    def table(lens):
        """{(length, code as read bit by bit, first bit first): symbol}"""
        out, code = {}, 0
        for ln in range(1, 16):
            for sym, l in enumerate(lens):
                if l == ln:
                    out[(ln, code)] = sym
                    code += 1
            code <<= 1
        return out

    def read(at, tab):
        code = 0
        for ln in range(1, 16):
            code = code << 1 | bits(at + ln - 1, 1)
            if (ln, code) in tab:
                return tab[(ln, code)], at + ln
        raise ValueError("no code")

    assert bits(1, 2) == 2
    nl, nd, ncl = 257 + bits(3, 5), 1 + bits(8, 5), 4 + bits(13, 4)
    at = 17
    cl = [0] * 19
    for i in range(ncl):
        cl[ob.CL_ORDER[i]] = bits(at, 3); at += 3
    ctab, lens = table(cl), []
    while len(lens) < nl + nd:
        sym, at = read(at, ctab)
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + bits(at, 2)); at += 2
        elif sym == 17:
            lens += [0] * (3 + bits(at, 3)); at += 3
        else:
            lens += [0] * (11 + bits(at, 7)); at += 7
    ltab, dtab = table(lens[:nl]), table(lens[nl:nl + nd])
    starts, out = {}, 0
    while at + 48 < n:
        starts[at] = out
        sym, at = read(at, ltab)
        if sym < 256:
            out += 1
        elif sym == 256:
            break
        else:
            run_ = int(ob.LEN_BASE[sym - 257]) + bits(at, int(ob.LEN_EXTRA[sym - 257])); at += int(ob.LEN_EXTRA[sym - 257])
            ds, at = read(at, dtab)
            at += int(ob.DIST_EXTRA[ds])
            out += run_
    return starts


def test_dynamic_block_resumed_at_a_token(emu, tmp_path):
    """other tables than the fixed ones: the state comes from a bit-walk over the block's own code, and the hand-over point must be a
    token start of that walk with the walk's byte count"""
    data, z = ob.one_dynamic_block(1, 300000)
    z = z[:len(z) * 3 // 4]
    starts = token_starts(z[2:])
    order = sorted(starts)
    bit = order[len(order) // 5]                                  # a token a fifth of the way in
    state = (16, 0, 16 + bit, starts[bit])
    rc, stats, hand, log = run(emu, tmp_path, z, data, state)
    assert rc == 0 and "MISMATCH" not in log, log
    tried, joined, redone = stats
    assert tried >= 8 and joined >= 1 and redone == 0, log
    assert hand is not None, log
    b, nbytes, hdr, hdr_bytes = hand
    assert (hdr, hdr_bytes) == (16, 0)
    assert starts.get(b - 16) == nbytes, hand
    assert nbytes > state[3] and 0 <= len(z) * 8 - b <= 2 * SEG * 8, (hand, len(z))
    # without cuts the same call ends as it always did: the pipeline stops in front of the block the input does not hold completely
    rc0, stats0, hand0, log0 = run(emu, tmp_path, z, data, state, cut=0)
    assert rc0 == 0 and stats0 is None and hand0 is None and "resume ok=2 done=0 state=16,0" in log0, log0


def test_other_tables_behind_the_anchor_end_as_without_cuts(emu, tmp_path):
    """the state stands in a dynamic block, most of the input behind it is a fixed block no search finds: the cuts do not stitch far
    from the end of the input, so nothing is handed over -- the call is redone the way it goes without cuts and ends as it does there"""
    data, z = ob.dynamic_then_fixed(3, 100000, 200000)
    z = z[:len(z) * 3 // 4]
    starts = token_starts(z[2:])
    order = sorted(starts)
    bit = order[len(order) // 5]
    state = (16, 0, 16 + bit, starts[bit])
    rc0, stats0, hand0, log0 = run(emu, tmp_path, z, data, state, cut=0)
    rc1, stats1, hand1, log1 = run(emu, tmp_path, z, data, state)
    verdict = [line for line in log1.splitlines() if line.startswith("resume ")]
    assert rc0 == rc1 == 0 and stats0 is None and hand0 is None and hand1 is None, log0 + log1
    assert stats1[0] >= 8 and stats1[2] == 1, log1
    assert verdict and verdict == [line for line in log0.splitlines() if line.startswith("resume ")], log0 + log1
    assert "resume ok=2" in verdict[0] and "state=16,0" not in verdict[0], "the redone call takes the dynamic block whole"
