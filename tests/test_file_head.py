"""csrc/file_head.hpp -- the host code that lays down everything between a PNG file's signature and its first IDAT -- against
tests/file_ref.py over a case table.  A stand-alone C++ program (tools/file_head_main.cpp, its own main) built twice with g++: plain, and
with -fsanitize=address,undefined; run as a subprocess with nothing preloaded.  Palettes and blobs live in allocations of exactly their
length, so a read behind them is seen."""
import shutil
import struct
import subprocess

import pytest

import file_ref
import pnghelp as ph

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}
DONE, E_ARGUMENT = 0, 65


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("file_head") / "file_head_main"
    flags = SANITIZE if request.param == "sanitized" else ()
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(out), str(ph.ROOT / "tools" / "file_head_main.cpp")],
                   check=True, capture_output=True, timeout=600)
    return out


def blob_bytes(n, seed):
    return bytes((seed + 7 * i + (i >> 8)) & 255 for i in range(n))


def case(fmt, width=5, height=3, interlaced=0, chunk_bytes=65544, key=None, fill=None, palette=(), before=(), after=()):
    """a case: the format by name, blobs as (type, len, seed)"""
    f = file_ref.FORMATS[fmt] if isinstance(fmt, str) else file_ref.Format(*fmt)
    return dict(fmt=f, width=width, height=height, interlaced=interlaced, chunk_bytes=chunk_bytes, key=key, fill=fill, palette=list(palette),
                before=list(before), after=list(after))


def line(c):
    f = c["fmt"]
    out = [c["width"], c["height"], f.depth, f.channels, f.indexed, f.bgr, c["interlaced"], c["chunk_bytes"]]
    for v in (c["key"], c["fill"]):
        out += [0, 0, 0, 0] if v is None else [1] + ([v, 0, 0] if isinstance(v, int) else list(v))
    out += [len(c["palette"])] + [x for p in c["palette"] for x in p]
    for group in (c["before"], c["after"]):
        out += [len(group)] + [x for name, n, seed in group for x in (struct.unpack(">I", name)[0], n, seed)]
    return " ".join(str(x) for x in out)


def expected(c):
    """-> (status, head bytes)"""
    f = c["fmt"]
    try:
        file_ref.body(b"x", c["chunk_bytes"])
        return DONE, file_ref.head(c["width"], c["height"], f.depth, f.channels, indexed=f.indexed, bgr=f.bgr, interlaced=c["interlaced"],
                                   palette=c["palette"], key=c["key"], fill=c["fill"],
                                   before=[(n, blob_bytes(k, s)) for n, k, s in c["before"]], after=[(n, blob_bytes(k, s)) for n, k, s in c["after"]])
    except file_ref.Refused:
        return E_ARGUMENT, b""


def run(prog, tmp_path, cases):
    (tmp_path / "cases.txt").write_text("\n".join(line(c) for c in cases) + "\n")
    r = subprocess.run([str(prog), str(tmp_path / "cases.txt"), str(tmp_path / "heads")], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    heads, pos, rows = (tmp_path / "heads").read_bytes(), 0, []
    for c, out in zip(cases, r.stdout.splitlines()):
        status, n, bound = (int(x) for x in out.split())
        rows.append((status, heads[pos:pos + n], bound))
        pos += n
    assert len(rows) == len(cases) and pos == len(heads)
    return rows


def check(prog, tmp_path, cases):
    for c, (status, head, bound) in zip(cases, run(prog, tmp_path, cases)):
        want_status, want = expected(c)
        assert (status, head) == (want_status, want), c
        chunks = -(-100000 // c["chunk_bytes"]) if want_status == DONE else 0
        assert bound == (8 + len(want) + 100000 + 12 * chunks + 12 if want_status == DONE else 0), c
    return [expected(c)[0] for c in cases]


PAL = [(10 * k % 256, (3 * k + 1) % 256, (250 - k) % 256, 255) for k in range(256)]


def test_every_format_with_and_without_key_and_fill(prog, tmp_path):
    cases = []
    for name, f in file_ref.FORMATS.items():
        kind = file_ref.kind_of(*f)
        top = (1 << f.depth) - 1
        pal = PAL[:1 << f.depth] if kind == "indexed" else []
        one = kind in ("v", "va")
        keys = [None] + ([top // 2 + 1 if one else (top, 0x12 if f.depth == 8 else 0x1234, 1)] if kind in ("v", "rgb") else [])
        fills = [None, 1 if kind == "indexed" else top if one else (2, top, 0x34 if f.depth == 8 else 0x3456)]
        for key in keys:
            for fill in fills:
                for interlaced in (0, 1):
                    cases.append(case(name, width=0x01020304, height=7, interlaced=interlaced, key=key, fill=fill, palette=pal))
        # a colour format's suggested palette: PLTE only when it is not empty
        if kind in ("rgb", "rgba"):
            cases.append(case(name, palette=PAL[:3], fill=(1, 2, 3)))
            cases.append(case(name, palette=PAL[:256]))
    assert set(check(prog, tmp_path, cases)) == {DONE}
    # the chunks and their order, stated once by hand: bgr8 with a key, a fill and a palette
    (status, head, _), = run(prog, tmp_path, [case("bgr8", width=2, height=1, key=(1, 2, 3), fill=(4, 5, 6), palette=[(7, 8, 9, 0)])])
    assert status == DONE and head == b"".join(file_ref.chunk(n, d) for n, d in (
        (b"CgBI", bytes([48, 0, 32, 6])), (b"IHDR", struct.pack(">IIBBBBB", 2, 1, 8, 2, 0, 0, 0)), (b"PLTE", bytes([7, 8, 9])),
        (b"bKGD", struct.pack(">HHH", 6, 5, 4)), (b"tRNS", struct.pack(">HHH", 3, 2, 1))))


def test_indexed_palettes_and_their_alphas(prog, tmp_path):
    cases = []
    for depth, counts in ((1, (1, 2)), (2, (1, 2, 4)), (4, (1, 2, 16)), (8, (1, 2, 256))):
        for count in counts:
            for which in ("opaque", "last", "first"):
                pal = [list(p) for p in PAL[:count]]
                if which != "opaque":
                    pal[-1 if which == "last" else 0][3] = 0x80
                cases.append(case(f"indexed{depth}", palette=[tuple(p) for p in pal], fill=count - 1))
    assert set(check(prog, tmp_path, cases)) == {DONE}
    rows = run(prog, tmp_path, cases[-3:])                       # 256 entries: no tRNS, all 256 alphas, one alpha
    lens = [len(dict(file_ref.parse(file_ref.SIG + r[1] + file_ref.chunk(b"IEND"))).get(b"tRNS", b"")) for r in rows]
    assert lens == [0, 256, 1]


def test_bgr_formats_with_a_key(prog, tmp_path):
    cases = [case("bgr8", key=(1, 2, 3)), case("bgr8", key=(255, 0, 7), fill=(9, 8, 7)), case("bgra8", fill=(1, 2, 3)), case("bgra8"),
             case("bgra8", palette=PAL[:5])]
    assert set(check(prog, tmp_path, cases)) == {DONE}


def test_blobs(prog, tmp_path):
    names = (b"gAMA", b"cHRM", b"iCCP", b"tEXt", b"prVt", b"zTXt", b"sPLT")
    many = [(names[k % len(names)], (0, 1, 70000, 5, 300)[k % 5], 11 * k) for k in range(12)]
    cases = []
    for before in ([], many[:1], many):
        for after in ([], many[3:4], many[::-1]):
            cases.append(case("rgb8", before=before, after=after, key=(1, 2, 3)))
            cases.append(case("indexed4", before=before, after=after, palette=PAL[:9], fill=2))
    for n in (0, 1, 70000):
        cases.append(case("v8", before=[(b"gAMA", n, 5)]))
        cases.append(case("v8", after=[(b"tIME", n, 6)]))
    assert set(check(prog, tmp_path, cases)) == {DONE}


def test_refusals(prog, tmp_path):
    cases = []
    for name in file_ref.OWNED + (b"IDaT", b"IDAt", b"Prvt", b"abcd", b"ABCD"):       # owned, reserved bit set, unknown critical
        cases.append(case("rgb8", before=[(name, 3, 1)]))
        cases.append(case("rgb8", after=[(b"gAMA", 4, 1), (name, 3, 1)]))
    cases += [case("indexed1", palette=PAL[:3]), case("indexed2", palette=PAL[:5]), case("indexed4", palette=PAL[:17]), case("indexed8", palette=[]),
              case("indexed8", palette=PAL + PAL[:1]), case("rgb8", palette=PAL + PAL[:1]), case("rgba16", palette=PAL + PAL[:1]),
              case("v8", palette=PAL[:1]), case("va16", palette=PAL[:2]),
              case("rgb8", width=0), case("rgb8", height=0), case("rgb8", chunk_bytes=0), case("rgb8", chunk_bytes=0x80000000),
              case((3, 1, 0, 0)), case((8, 5, 0, 0)), case((16, 1, 1, 0)), case((16, 3, 0, 1)), case((4, 3, 0, 0)), case((8, 2, 0, 1)),
              case("va8", key=1), case("rgba8", key=(1, 2, 3)), case("indexed8", palette=PAL[:4], key=1), case("bgra8", key=(1, 2, 3)),
              case("rgb8", key=(256, 0, 0)), case("v8", fill=256), case("v2", fill=4), case("indexed4", palette=PAL[:4], fill=4)]
    assert set(check(prog, tmp_path, cases)) == {E_ARGUMENT}
    # ... and the largest values that pass
    cases = [case("rgb8", chunk_bytes=1), case("rgb8", chunk_bytes=0x7fffffff), case("v2", fill=3), case("indexed4", palette=PAL[:4], fill=3),
             case("rgb16", key=(65535, 0, 1)), case("rgb8", before=[(b"prVt", 2, 1)])]
    assert set(check(prog, tmp_path, cases)) == {DONE}
